"""Test helper: the numpy / pure-Python specification of the molecule strings written on the device
(csrc/gi_smiles.hip, ``graphinvent_amd.analyze.smiles`` / ``write_smi``), an independent reader of such strings, and a
comparison of two labelled graphs.  The device must match ``write`` byte for byte.

THE STRING IS A FAITHFUL SPELLING OF THE LABELLED GRAPH in an OpenSMILES subset, NOT RDKit's canonical SMILES: no
aromaticity, no stereo, the hydrogen counts are the rules' fill or the stored ones.

``write`` (the grammar; include/graphinvent_amd.h states it for ``gi_mol_smiles``):

  status      tests/valence_model.judge's bits without VAL_H_MISMATCH (SMI_EMPTY = VAL_EMPTY, and so on), plus
              SMI_RING_LIMIT and SMI_TRUNCATED.  A malformed molecule (``VM.MALFORMED``), SMI_EMPTY, SMI_SELF_LOOP,
              SMI_AROMATIC and SMI_RING_LIMIT give an empty string, length 0 and atom_pos -1; SMI_TRUNCATED gives an
              empty text and atom_pos -1 with ``length`` = the bytes needed
  key         atoms are ordered by (rank[i], i), the input index without a rank
  atom token  bare symbol when the symbol is one of B C N O P S F Cl Br I, the charge is 0 and h equals the OpenSMILES
              implicit count for the bond-order sum x (v - x, v the smallest normal valence >= x, 0 without one); else
              ``[`` symbol, ``H`` if h >= 1, h if h >= 2, ``+`` / ``-``, the magnitude if >= 2, ``]``; type "H" is
              ``[H]`` with its charge, never a count
  order       components by their lowest-key atom, joined by ``.``; each walked depth-first from that atom, neighbours
              in ascending key; unvisited when reached: a tree child, visited and not the parent: a ring bond
  at an atom  the token; ring closings in ascending pre-order index of the partner (bond symbol, number; the number is
              free again at once); ring openings in the same order (the smallest free number >= 1, no bond symbol);
              the children in visiting order, all but the last in parentheses, the bond symbol in front of the child's
              token inside the parenthesis.  Numbers 1-9 are a digit, 10-99 ``%nn``; a single bond is elided, a double
              bond is ``=``, a triple bond ``#``

``read`` is written from the OpenSMILES text alone: it shares no code and no table object with ``write``."""
import numpy as np

from tests import valence_model as VM

SMI_EMPTY, SMI_SELF_LOOP, SMI_OVER, SMI_FRAGMENTS, SMI_AROMATIC = 128, 256, 512, 1024, 2048
SMI_RING_LIMIT, SMI_TRUNCATED = 8192, 16384
SMI_MAX_LEN = 8192
NO_STRING = VM.MALFORMED | SMI_EMPTY | SMI_SELF_LOOP | SMI_AROMATIC | SMI_RING_LIMIT

ORGANIC = {"B": (3,), "C": (4,), "N": (3, 5), "O": (2,), "P": (3, 5), "S": (2, 4, 6), "F": (1,), "Cl": (1,),
           "Br": (1,), "I": (1,)}
BOND_SYMBOL = {2: "", 4: "=", 6: "#"}


def default_max_len(N):
    return (12 * N + 4 + 15) // 16 * 16


def atom_token(symbol, charge, h, x):
    if symbol == "H":
        h = 0
    elif symbol in ORGANIC and charge == 0:
        fits = [v for v in ORGANIC[symbol] if v >= x]
        if h == (fits[0] - x if fits else 0):
            return symbol
    tok = "[" + symbol
    if h >= 1:
        tok += "H" + (str(h) if h >= 2 else "")
    if charge:
        tok += ("+" if charge > 0 else "-") + (str(abs(charge)) if abs(charge) >= 2 else "")
    return tok + "]"


def ring_number(k):
    return str(k) if k < 10 else "%" + str(k)


def write(nodes, edges, n_given, rules, rank=None, hydrogens=None, max_len=None):
    """One molecule -> dict(text (bytes, without the padding), length, status, atom_pos [N] int32)."""
    nodes, edges = np.asarray(nodes), np.asarray(edges)
    N = nodes.shape[0]
    A, C, H = rules.groups
    max_len = default_max_len(N) if max_len is None else max_len
    hydrogens = ("stored" if H else "fill") if hydrogens is None else hydrogens
    assert hydrogens in ("fill", "stored") and (hydrogens == "fill" or H)
    v = VM.judge(nodes, edges, n_given, rules)
    status = int(v["status"]) & ~VM.VAL_H_MISMATCH
    out = dict(text=b"", length=0, status=status, atom_pos=np.full(N, -1, np.int32))
    if status & NO_STRING:
        return out
    n = int(v["desc"][0])
    nz_n, nz_e = nodes != 0, edges != 0
    order2 = {}                                                         # (i, j) -> twice the bond order
    for i, j, t in zip(*np.nonzero(nz_e[:n, :n])):
        order2[(int(i), int(j))] = rules.order2[t]
    tokens = []
    for i in range(n):
        a = int(np.flatnonzero(nz_n[i, :A])[0])
        c = int(np.flatnonzero(nz_n[i, A:A + C])[0])
        h = int(v["atom_h"][i])
        if hydrogens == "stored":
            h = rules.h_values[int(np.flatnonzero(nz_n[i, A + C:A + C + H])[0])]
        x = (sum(o for (p, _), o in order2.items() if p == i) + 1) // 2
        tokens.append(atom_token(rules.atom_types[a], rules.formal_charge[c], h, x))
    key = [(int(rank[i]) if rank is not None else i, i) for i in range(n)]
    by_key = sorted(range(n), key=lambda i: key[i])
    nbrs = [sorted((j for j in range(n) if (i, j) in order2), key=lambda j: key[j]) for i in range(n)]

    # the walk: pre-order, tree parent, children in visiting order
    pre, parent, children, roots = {}, {}, {i: [] for i in range(n)}, []
    for root in by_key:
        if root in pre:
            continue
        roots.append(root)
        pre[root], parent[root] = len(pre), None
        stack = [(root, iter(nbrs[root]))]
        while stack:
            i, it = stack[-1]
            for j in it:
                if j not in pre:
                    pre[j], parent[j] = len(pre), i
                    children[i].append(j)
                    stack.append((j, iter(nbrs[j])))
                    break
            else:
                stack.pop()
    atoms = sorted(range(n), key=lambda i: pre[i])

    # ring numbers, in pre-order
    ring_text, free, number = {}, [True] * 100, {}
    for i in atoms:
        rings = sorted((j for j in nbrs[i] if j != parent[i] and parent[j] != i), key=lambda j: pre[j])
        text = ""
        for j in rings:
            if pre[j] < pre[i]:
                k = number.pop((j, i))
                text += BOND_SYMBOL[order2[(i, j)]] + ring_number(k)
                free[k] = True
        for j in rings:
            if pre[j] > pre[i]:
                k = next((k for k in range(1, 100) if free[k]), None)
                if k is None:
                    out["status"] |= SMI_RING_LIMIT
                    return out
                free[k], number[(i, j)] = False, k
                text += ring_number(k)
        ring_text[i] = text

    pos, parts = np.full(N, -1, np.int32), []

    def emit(i, at):
        """Atom i and its subtree, the first byte at `at`; -> the bytes written."""
        start = at
        lead = BOND_SYMBOL[order2[(i, parent[i])]] if parent[i] is not None else ""
        parts.append(lead)
        at += len(lead)
        pos[i] = at
        parts.append(tokens[i] + ring_text[i])
        at += len(tokens[i]) + len(ring_text[i])
        for c in children[i]:
            if c != children[i][-1]:
                parts.append("(")
                at += 1 + emit(c, at + 1)
                parts.append(")")
                at += 1
            else:
                at += emit(c, at)
        return at - start

    import sys
    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 4 * N + 200))
    try:
        at = 0
        for r in roots:
            if at:
                parts.append(".")
                at += 1
            at += emit(r, at)
    finally:
        sys.setrecursionlimit(limit)
    text = "".join(parts).encode("ascii")
    assert len(text) == at
    out["length"] = len(text)
    if len(text) > max_len:
        out["status"] |= SMI_TRUNCATED
        return out
    out["text"], out["atom_pos"] = text, pos
    return out


def write_batch(nodes, edges, n_nodes, rules, rank=None, hydrogens=None, max_len=None):
    """Batch model of ``analyze.smiles`` -> dict(text [G, max_len] uint8, length / status [G] int32, atom_pos [G, N]
    int32, strings: list of str)."""
    nodes, edges = np.asarray(nodes), np.asarray(edges)
    G, N = nodes.shape[:2]
    max_len = default_max_len(N) if max_len is None else max_len
    out = dict(text=np.zeros((G, max_len), np.uint8), length=np.zeros(G, np.int32), status=np.zeros(G, np.int32),
               atom_pos=np.full((G, N), -1, np.int32), strings=[])
    for g in range(G):
        one = write(nodes[g], edges[g], None if n_nodes is None else n_nodes[g], rules,
                    None if rank is None else rank[g], hydrogens, max_len)
        out["text"][g, :len(one["text"])] = np.frombuffer(one["text"], np.uint8)
        out["length"][g], out["status"][g], out["atom_pos"][g] = one["length"], one["status"], one["atom_pos"]
        out["strings"].append(one["text"].decode("ascii"))
    return out


# ---- the reader: OpenSMILES, written apart from the writer --------------------------------------------------------
_NORMAL = dict(B=[3], C=[4], N=[3, 5], O=[2], P=[3, 5], S=[2, 4, 6], F=[1], Cl=[1], Br=[1], I=[1])
_TWO_LETTER_BARE = ("Cl", "Br")
_BOND_CHARS = {"-": 1, "=": 2, "#": 3}


class SmilesError(ValueError):
    pass


def read(s):
    """-> dict(elements [str], charges [int], hydrogens [int], bonds {(i, j): order}, i < j) of a SMILES string in the
    subset: bracket atoms with H counts and charges, the organic subset with implicit hydrogens, ``-`` ``=`` ``#``,
    branches, ring digits, ``%nn`` and ``.``."""
    elements, charges, hcount, bracket, bonds = [], [], [], [], {}
    open_rings = {}                                                     # number -> (atom, order or None)
    branch, prev, pending, k = [], None, None, 0

    def bond(a, b, order):
        if a == b or (min(a, b), max(a, b)) in bonds:
            raise SmilesError(f"bond {a}-{b} twice or to itself in {s!r}")
        bonds[(min(a, b), max(a, b))] = order

    def new_atom(el, q, h, br):
        nonlocal prev, pending
        elements.append(el); charges.append(q); hcount.append(h); bracket.append(br)
        me = len(elements) - 1
        if prev is not None:
            bond(prev, me, pending or 1)
        elif pending is not None:
            raise SmilesError(f"a bond without a left atom in {s!r}")
        prev, pending = me, None

    while k < len(s):
        ch = s[k]
        if ch == "[":
            end = s.find("]", k)
            if end < 0:
                raise SmilesError(f"unclosed bracket in {s!r}")
            body, j = s[k + 1:end], 0
            if not body or not body[0].isupper():
                raise SmilesError(f"bracket atom {body!r} in {s!r}")
            j = 2 if len(body) > 1 and body[1].islower() else 1
            el, h, q = body[:j], 0, 0
            if j < len(body) and body[j] == "H":
                j += 1
                d = j
                while d < len(body) and body[d].isdigit():
                    d += 1
                h = int(body[j:d]) if d > j else 1
                j = d
            if j < len(body) and body[j] in "+-":
                sign = 1 if body[j] == "+" else -1
                j += 1
                d = j
                while d < len(body) and body[d].isdigit():
                    d += 1
                q = sign * (int(body[j:d]) if d > j else 1)
                j = d
            if j != len(body):
                raise SmilesError(f"bracket atom {body!r} in {s!r}")
            new_atom(el, q, h, True)
            k = end + 1
        elif ch.isupper():
            el = s[k:k + 2] if s[k:k + 2] in _TWO_LETTER_BARE else ch
            if el not in _NORMAL:
                raise SmilesError(f"{el!r} outside a bracket in {s!r}")
            new_atom(el, 0, None, False)
            k += len(el)
        elif ch in _BOND_CHARS:
            if pending is not None:
                raise SmilesError(f"two bond symbols in {s!r}")
            pending = _BOND_CHARS[ch]
            k += 1
        elif ch.isdigit() or ch == "%":
            if ch == "%":
                if not s[k + 1:k + 3].isdigit() or len(s[k + 1:k + 3]) != 2:
                    raise SmilesError(f"%nn in {s!r}")
                num, k = int(s[k + 1:k + 3]), k + 3
            else:
                num, k = int(ch), k + 1
            if prev is None:
                raise SmilesError(f"a ring digit without an atom in {s!r}")
            if num in open_rings:
                other, order = open_rings.pop(num)
                if order is not None and pending is not None and order != pending:
                    raise SmilesError(f"ring {num} closes with another bond in {s!r}")
                bond(other, prev, pending or order or 1)
            else:
                open_rings[num] = (prev, pending)
            pending = None
        elif ch == "(":
            if prev is None:
                raise SmilesError(f"a branch without an atom in {s!r}")
            branch.append(prev)
            k += 1
        elif ch == ")":
            if not branch or pending is not None:
                raise SmilesError(f"')' in {s!r}")
            prev = branch.pop()
            k += 1
        elif ch == ".":
            if pending is not None or prev is None:
                raise SmilesError(f"'.' in {s!r}")
            prev = None
            k += 1
        else:
            raise SmilesError(f"{ch!r} in {s!r}")
    if open_rings or branch or pending is not None:
        raise SmilesError(f"unfinished ring, branch or bond in {s!r}")
    total = [0] * len(elements)
    for (a, b), order in bonds.items():
        total[a] += order
        total[b] += order
    for i, el in enumerate(elements):
        if not bracket[i]:                                              # implicit hydrogens: up to the next normal valence
            room = [v for v in _NORMAL[el] if v >= total[i]]
            hcount[i] = room[0] - total[i] if room else 0
    return dict(elements=elements, charges=charges, hydrogens=hcount, bonds=bonds)


def graph_of(nodes, edges, n_given, rules, hydrogens=None):
    """The labelled graph of a (sound) molecule tensor in ``read``'s form, the hydrogens as ``write`` takes them."""
    nodes, edges = np.asarray(nodes), np.asarray(edges)
    A, C, H = rules.groups
    hydrogens = ("stored" if H else "fill") if hydrogens is None else hydrogens
    v = VM.judge(nodes, edges, n_given, rules)
    n = int(v["desc"][0])
    el = [rules.atom_types[int(np.flatnonzero(nodes[i, :A])[0])] for i in range(n)]
    q = [rules.formal_charge[int(np.flatnonzero(nodes[i, A:A + C])[0])] for i in range(n)]
    if hydrogens == "stored":
        h = [rules.h_values[int(np.flatnonzero(nodes[i, A + C:A + C + H])[0])] for i in range(n)]
    else:
        h = [int(x) for x in v["atom_h"][:n]]
    h = [0 if e == "H" else x for e, x in zip(el, h)]                   # "[H]" never carries a count
    bonds = {}
    for i, j, t in zip(*np.nonzero(edges[:n, :n])):
        if i < j:
            bonds[(int(i), int(j))] = rules.order2[t] // 2
    return dict(elements=el, charges=q, hydrogens=h, bonds=bonds)


def same(a, b):
    """Whether two graphs (``read``'s form) are isomorphic with equal elements, charges, hydrogen counts and bond
    orders."""
    import networkx as nx
    if len(a["elements"]) != len(b["elements"]) or len(a["bonds"]) != len(b["bonds"]):
        return False

    def build(m):
        g = nx.Graph()
        for i, label in enumerate(zip(m["elements"], m["charges"], m["hydrogens"])):
            g.add_node(i, label=label)
        for (i, j), order in m["bonds"].items():
            g.add_edge(i, j, order=order)
        return g

    return nx.is_isomorphic(build(a), build(b), node_match=lambda x, y: x["label"] == y["label"],
                            edge_match=lambda x, y: x["order"] == y["order"])


def read_smi(path):
    """-> (header, [(string, name)]) of a ``.smi`` file."""
    with open(path) as f:
        lines = f.read().splitlines()
    return lines[0], [tuple(line.split(" ")) for line in lines[1:]]
