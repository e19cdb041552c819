"""Test helper: the pure-Python specification of the SMILES reader WITH AROMATIC INPUT (csrc/gi_smiles_read.hip,
``gi_smiles_read_arom``; ``graphinvent_amd.analyze.read_smiles(..., aromatic="kekulize")``).  The device must match
``read_batch`` in every byte of every output.  With ``aromatic=False`` this reader is tests/smiles_read_model.py, stage
by stage; with ``aromatic=True`` it is the same reader on every string without a lowercase atom token and without ``:``.

THE KEKULISATION IS OURS, NOT RDKit'S: no ring perception, no aromaticity perception, no canonical choice.  What the
option adds, stage by stage:

  A bytes  outside a bracket ``b c n o p s`` start an (aromatic) atom and ``:`` is a bond symbol; any other small letter
           stays RD_SYNTAX.  No RD_AROMATIC is ever set.
  B atoms  a bracket atom whose symbol starts with a small letter: the symbol (one small letter, and a second one if a
           small letter follows) must be one of ``b c n o p s se as`` (RD_SYNTAX otherwise) and is looked up
           CAPITALISED; the rest of the token as before.  An atom is AROMATIC when its symbol starts with a small letter.
  C walk   a bond WITHOUT a symbol (on either end, for a ring bond) between two aromatic atoms is AROMATIC-MARKED, and
           so is ``:`` between two aromatic atoms; ``:`` next to an atom that is not aromatic: RD_UNSUPPORTED (after
           RD_RING_ORDER / RD_SELF_LOOP / RD_MULTI_BOND, which are checked first as before; ``:`` on one end of a ring
           bond and another symbol on the other is RD_RING_ORDER).  ``-`` ``=`` ``#`` mean what they say.  An
           aromatic-marked bond counts as a bond for RD_MULTI_BOND and RD_FRAGMENTS; its type is not looked up here.
  C2       only without an error bit so far.  sigma(i) = the bond-order sum with every aromatic-marked bond counted 1.
           An aromatic atom NEEDS a double bond when: bare, sigma is not a normal valence of its element (``NORMAL``)
           and a larger one exists; bracket, sigma + stated H is not in ``allowed[type][charge]`` and a larger allowed
           valence exists.  No other atom needs one.  The CANDIDATE graph: the aromatic-marked bonds between two needing
           atoms.  A perfect matching of the needing atoms in it is looked for (``match``: greedy in ascending index,
           then one breadth-first augmenting-path search with blossom contraction per free needing atom in ascending
           index, neighbours in ascending index; the first search that fails ends it).  None: RD_KEKULE.  Otherwise
           matched bonds get the double type (order2 == 4), every other aromatic-marked bond the single type; a type
           that is needed and missing: RD_BOND_ORDER.
  D atoms  as before on the Kekule bonds; a bare aromatic symbol is capitalised before ``NORMAL`` is asked.
  out      RD_KEKULIZED (informational) when the string had an aromatic atom and no error bit."""
import numpy as np

from tests import smiles_read_model as RM
from tests.smiles_read_model import (MAX_DEPTH, MAX_RINGS, NORMAL, RD_AROMATIC, RD_BOND_ORDER, RD_CHARGE, RD_ELEMENT,
                                     RD_EMPTY, RD_FRAGMENTS, RD_HCOUNT, RD_MULTI_BOND, RD_OVER, RD_RING_OPEN,
                                     RD_RING_ORDER, RD_SELF_LOOP, RD_STEREO, RD_STEREO_DROPPED, RD_SYNTAX, RD_TOO_MANY,
                                     RD_UNSUPPORTED, T_ATOM, T_BOND1, T_BOND2, T_BOND3, T_CLOSE, T_DIGIT, T_DOT, T_OPEN,
                                     T_PERCENT, T_SKIP, _digit, _lower, pack)

RD_KEKULE, RD_KEKULIZED = 1 << 26, 1 << 27
RD_INFO = RM.RD_INFO | RD_KEKULIZED
RD_ERROR = RM.RD_ERROR | RD_KEKULE
T_BONDA = 10                                                                # ':'; the walk's pending code for it is 4
AROMATIC_BARE = b"bcnops"
AROMATIC_BRACKET = (b"b", b"c", b"n", b"o", b"p", b"s", b"se", b"as")       # OpenSMILES' list


def classify(s, drop_stereo, aromatic):
    """Stage A -> (class of every byte, flags, offsets of the atom tokens)."""
    cls, flags, starts = RM.classify(s, drop_stereo)
    if not aromatic or not flags & RD_AROMATIC:
        return cls, flags, starts
    flags &= ~RD_AROMATIC                                                   # the bytes that set it become tokens
    inside = False
    for k, b in enumerate(s):
        if b in b"[]":
            inside = b == ord("[")
        elif not inside and b in AROMATIC_BARE:
            cls[k] = T_ATOM
        elif not inside and b == ord(":"):
            cls[k] = T_BONDA
    return cls, flags, [k for k, c in enumerate(cls) if c == T_ATOM]


def parse_atom(s, k, drop_stereo, aromatic):
    """Stage B, the token at offset k -> (flags, symbol bytes CAPITALISED, charge, stated H or None, aromatic)."""
    if not aromatic:
        return RM.parse_atom(s, k, drop_stereo) + (False,)
    if s[k] != ord("["):
        if _lower(s[k]):
            return 0, s[k:k + 1].upper(), 0, None, True
        return RM.parse_atom(s, k, drop_stereo) + (False,)
    if k + 1 >= len(s) or not _lower(s[k + 1]):
        return RM.parse_atom(s, k, drop_stereo) + (False,)
    j = k + 2
    if j < len(s) and _lower(s[j]):
        j += 1
    sym = s[k + 1:j]
    if sym not in AROMATIC_BRACKET:
        return RD_SYNTAX, b"", 0, 0, True
    # the rest of the token is the old grammar's: read it behind a capital in the small letters' place
    flags, _, q, h = RM.parse_atom(b"[" + sym.capitalize() + s[j:], 0, drop_stereo)
    return flags, sym.capitalize(), q, h, True


def match(n, need, cand, counters=None):
    """The perfect matching of C2 -> mate [n] (-1: free) or None.  ``cand[i]``: the candidate neighbours of i,
    ascending.  ``counters``: a dict whose 'greedy', 'searches', 'augmentations' and 'blossoms' are counted up."""
    count = counters if counters is not None else {}
    for key in ("greedy", "searches", "augmentations", "blossoms"):
        count.setdefault(key, 0)
    mate = [-1] * n
    for i in range(n):                                                      # the greedy pass
        if need[i] and mate[i] < 0:
            for j in cand[i]:
                if mate[j] < 0:
                    mate[i], mate[j] = j, i
                    count["greedy"] += 1
                    break

    def search(root):
        used, parent, base = [False] * n, [-1] * n, list(range(n))
        used[root] = True
        queue, head = [root], 0

        def lca(a, b):
            seen = [False] * n
            while True:
                a = base[a]
                seen[a] = True
                if mate[a] < 0:
                    break
                a = parent[mate[a]]
            while True:
                b = base[b]
                if seen[b]:
                    return b
                b = parent[mate[b]]

        def mark_path(v, b, child, blossom):
            while base[v] != b:
                blossom[base[v]] = blossom[base[mate[v]]] = True
                parent[v] = child
                child = mate[v]
                v = parent[mate[v]]

        while head < len(queue):
            v = queue[head]
            head += 1
            for to in cand[v]:
                if base[v] == base[to] or mate[v] == to:
                    continue
                if to == root or (mate[to] >= 0 and parent[mate[to]] >= 0):
                    cur = lca(v, to)
                    blossom = [False] * n
                    mark_path(v, cur, to, blossom)
                    mark_path(to, cur, v, blossom)
                    count["blossoms"] += 1
                    for i in range(n):
                        if blossom[base[i]]:
                            base[i] = cur
                            if not used[i]:
                                used[i] = True
                                queue.append(i)
                elif parent[to] < 0:
                    parent[to] = v
                    if mate[to] < 0:
                        return to, parent
                    used[mate[to]] = True
                    queue.append(mate[to])
        return -1, parent

    for root in range(n):
        if need[root] and mate[root] < 0:
            count["searches"] += 1
            v, parent = search(root)
            if v < 0:
                return None
            count["augmentations"] += 1
            while v >= 0:
                pv = parent[v]
                nxt = mate[pv]
                mate[v], mate[pv] = pv, v
                v = nxt
    return mate


def read_one(row, length, rules, N, Fn, Fe, none_chirality=0, drop_stereo=False, aromatic=False, trace=None):
    """One string -> dict(nodes, edges, n_nodes, status, atom_pos) as ``smiles_read_model.read_one``.  ``trace``: a dict
    that receives the intermediate results (``n``, ``is_arom``, ``written`` {(a, b): order} of the bonds with a symbol
    or outside the aromatic atoms, ``marked`` the aromatic-marked pairs, ``need``, ``cand``, ``mate``, ``counters``)."""
    A, C, H = rules.groups
    assert A + C + H <= Fn and (A + C + H == Fn or 0 <= none_chirality < Fn - (A + C + H)) and len(rules.order2) == Fe
    row = bytes(bytearray(np.asarray(row, np.uint8)))
    nodes, edges = np.zeros((N, Fn), np.int8), np.zeros((N, N, Fe), np.int8)
    pos = np.full(N, -1, np.int32)
    trace = {} if trace is None else trace

    def result(status, n):
        if status & RD_ERROR:
            nodes[:], edges[:], pos[:] = 0, 0, -1
            n = n if status & RD_TOO_MANY else 0
        return dict(nodes=nodes, edges=edges, n_nodes=n, status=status, atom_pos=pos)

    if length is None:
        length = row.index(0) if 0 in row else len(row)
    elif not 0 <= length <= len(row):
        return result(RD_SYNTAX, 0)
    if length == 0:
        return result(RD_EMPTY, 0)
    s = row[:length]
    cls, status, starts = classify(s, drop_stereo, aromatic)
    n = len(starts)
    if n > N:
        return result(status | RD_TOO_MANY, n)

    # B: the atom tokens
    a_idx, c_idx, stated, is_arom = [0] * n, [0] * n, [None] * n, [False] * n
    symbols = [t.encode("ascii") for t in rules.atom_types]
    for i, k in enumerate(starts):
        flags, sym, q, stated[i], is_arom[i] = parse_atom(s, k, drop_stereo, aromatic)
        if not flags & RD_ERROR:
            if sym in symbols:
                a_idx[i] = symbols.index(sym)
            else:
                flags |= RD_ELEMENT
            if q in rules.formal_charge:
                c_idx[i] = rules.formal_charge.index(q)
            else:
                flags |= RD_CHARGE
        status |= flags
    if status & RD_ERROR:
        return result(status, 0)

    # C: the walk
    order, marked = {}, set()                                               # (i, j), both ways
    root = list(range(n))

    def find(x):
        while root[x] != x:
            x = root[x]
        return x

    def bond(a, b, o):                                                      # o: 0 no symbol, 1 .. 3, 4 ':'
        if a == b:
            return RD_SELF_LOOP
        if (a, b) in order or (a, b) in marked:
            return RD_MULTI_BOND
        both = is_arom[a] and is_arom[b]
        if o == 4 and not both:
            return RD_UNSUPPORTED
        if o in (0, 4) and both:
            marked.update(((a, b), (b, a)))
        else:
            o = o or 1
            if 2 * o not in rules.order2:
                return RD_BOND_ORDER
            order[(a, b)] = order[(b, a)] = o
        ra, rb = find(a), find(b)
        root[max(ra, rb)] = min(ra, rb)
        return 0

    pend = {T_BOND1: 1, T_BOND2: 2, T_BOND3: 3, T_BONDA: 4}
    ring_atom, ring_order = [-1] * MAX_RINGS, [0] * MAX_RINGS
    stack, prev, pending, atoms, after_open, err, k = [], -1, 0, 0, False, 0, 0
    while k < length and not err:
        t = cls[k]
        step = 1
        if t == T_SKIP:
            k += 1
            continue
        if t == T_ATOM:
            if prev >= 0:
                err = bond(prev, atoms, pending)
            elif pending:
                err = RD_SYNTAX
            prev, pending, atoms = atoms, 0, atoms + 1
        elif t in pend:
            if pending or prev < 0:
                err = RD_SYNTAX
            pending = pend[t]
        elif t in (T_DIGIT, T_PERCENT):
            num = s[k] - 48
            if t == T_PERCENT:
                if k + 2 < length and _digit(s[k + 1]) and _digit(s[k + 2]):
                    num, step = 10 * (s[k + 1] - 48) + s[k + 2] - 48, 3
                else:
                    err = RD_SYNTAX
            if not err and prev < 0:
                err = RD_SYNTAX
            if not err:
                if ring_atom[num] >= 0:
                    other, o = ring_atom[num], ring_order[num]
                    ring_atom[num] = -1
                    if o and pending and o != pending:
                        err = RD_RING_ORDER
                    else:
                        err = bond(other, prev, pending or o)
                else:
                    ring_atom[num], ring_order[num] = prev, pending
                pending = 0
        elif t == T_OPEN:
            if prev < 0 or pending or after_open or len(stack) == MAX_DEPTH:
                err = RD_SYNTAX
            else:
                stack.append(prev)
        elif t == T_CLOSE:
            if not stack or pending or after_open:
                err = RD_SYNTAX
            else:
                prev = stack.pop()
        elif t == T_DOT:
            if prev < 0 or pending:
                err = RD_SYNTAX
            prev = -1
        after_open = t == T_OPEN
        k += step
    if not err:
        if stack or pending:
            err = RD_SYNTAX
        elif any(a >= 0 for a in ring_atom):
            err = RD_RING_OPEN
    status |= err
    if not err and len({find(i) for i in range(n)}) > 1:
        status |= RD_FRAGMENTS
    if status & RD_ERROR:
        return result(status, 0)

    # C2: which atoms need a double bond; the matching; the Kekule bonds
    trace.update(n=n, is_arom=list(is_arom), written=dict(order), marked=set(marked))
    if marked or any(is_arom):
        need = [False] * n
        for i in range(n):
            if not is_arom[i]:
                continue
            sigma = sum(o for (a, _), o in order.items() if a == i) + sum(1 for (a, _) in marked if a == i)
            if stated[i] is None:
                x, table = sigma, NORMAL[symbols[a_idx[i]]]
            else:
                x, table = sigma + stated[i], rules.allowed[a_idx[i]][c_idx[i]]
            need[i] = x not in table and any(v > x for v in table)
        cand = [sorted(b for (a, b) in marked if a == i and need[b]) if need[i] else [] for i in range(n)]
        counters = {}
        mate = match(n, need, cand, counters)
        trace.update(need=need, cand=cand, mate=mate, counters=counters)
        if mate is None:
            return result(status | RD_KEKULE, 0)
        for (a, b) in marked:
            o = 2 if mate[a] == b else 1
            if 2 * o not in rules.order2:
                status |= RD_BOND_ORDER
            order[(a, b)] = o
        if status & RD_ERROR:
            return result(status, 0)

    # D: hydrogens, the implicit-H entry, the valence
    h_idx = [0] * n
    for i in range(n):
        x = sum(o for (a, _), o in order.items() if a == i)
        if stated[i] is None:
            fits = [v for v in NORMAL[symbols[a_idx[i]]] if v >= x]
            h = fits[0] - x if fits else 0
        else:
            h = stated[i]
        if H:
            if h in rules.h_values:
                h_idx[i] = rules.h_values.index(h)
            else:
                status |= RD_HCOUNT
        if not any(v >= x for v in rules.allowed[a_idx[i]][c_idx[i]]):
            status |= RD_OVER
    if status & RD_ERROR:
        return result(status, 0)
    if any(is_arom):
        status |= RD_KEKULIZED

    for i in range(n):
        nodes[i, a_idx[i]] = nodes[i, A + c_idx[i]] = 1
        if H:
            nodes[i, A + C + h_idx[i]] = 1
        if A + C + H < Fn:
            nodes[i, A + C + H + none_chirality] = 1
        pos[i] = starts[i]
    for (a, b), o in order.items():
        edges[a, b, rules.order2.index(2 * o)] = 1
    return result(status, n)


def read_batch(text, length, rules, N, Fn=None, Fe=None, none_chirality=0, drop_stereo=False, aromatic=False,
               traces=None):
    """Batch model of ``analyze.read_smiles(..., aromatic=...)`` -> the dict of ``smiles_read_model.read_batch``.
    ``traces``: a list that receives one ``trace`` dict per string."""
    if not isinstance(text, np.ndarray):
        text, length = pack(text)
    Fn = sum(rules.groups) if Fn is None else Fn
    Fe = len(rules.order2) if Fe is None else Fe
    G = len(text)
    out = dict(nodes=np.zeros((G, N, Fn), np.int8), edges=np.zeros((G, N, N, Fe), np.int8),
               n_nodes=np.zeros(G, np.int32), status=np.zeros(G, np.int32), atom_pos=np.full((G, N), -1, np.int32))
    for g in range(G):
        trace = {}
        one = read_one(text[g], None if length is None else int(length[g]), rules, N, Fn, Fe, none_chirality,
                       drop_stereo, aromatic, trace)
        if traces is not None:
            traces.append(trace)
        for name, value in one.items():
            out[name][g] = value
    return out
