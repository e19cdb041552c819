"""Test helper: the pure-Python specification of the SMILES reader on the device (csrc/gi_smiles_read.hip,
``graphinvent_amd.analyze.read_smiles`` / ``read_smi``).  The device must match ``read_batch`` in every byte of every
output.  It is written apart from ``tests/smiles_model.py::read``, which stays the independent witness: this one works
in the kernel's stages, on bytes, and produces tensors and status bits; that one raises on the first thing it does not
like and returns a dict.

THE READER TAKES THE WRITER'S SUBSET of OpenSMILES (include/graphinvent_amd.h states it at ``gi_smiles_read``): bracket
atoms ``[`` symbol ``H`` count sign magnitude ``]``, the bare organic atoms, ``-`` ``=`` ``#``, branches, ring digits and
``%nn``, ``.``.  No aromatic atoms or bonds and no stereo: such strings get a status bit and no molecule.  Atoms are
numbered in string order.

The stages, and which status bits each can set (a later stage runs only as stated, so that the bits of a string with
several defects are defined):

  length   ``length`` outside [0, max_len]: RD_SYNTAX, nothing else.  Without ``length`` the string ends at its first
           zero byte.  An empty string: RD_EMPTY, nothing else.
  A bytes  every byte by itself.  A byte is INSIDE a bracket when the last ``[`` or ``]`` before it is a ``[``.
           ``[`` inside: RD_SYNTAX; ``]`` outside: RD_SYNTAX.  Outside: B C N O P S F I start an atom (``l`` after ``C``
           and ``r`` after ``B`` belong to it); any other capital (bare ``H`` too): RD_SYNTAX; b c n o p s and ``:``:
           RD_AROMATIC; ``/`` ``\\``: RD_STEREO, or with drop_stereo RD_STEREO_DROPPED and a single bond; ``$`` ``*``:
           RD_UNSUPPORTED; ``- = # ( ) . %`` and digits are the walk's tokens; anything else: RD_SYNTAX.  ``[`` outside
           starts an atom.  More than N atoms: RD_TOO_MANY, ``n_nodes`` = the atoms needed, nothing below runs.
  B atoms  every bracket atom by itself: isotope digits, ``*``, ``++`` / ``--``, ``:class``: RD_UNSUPPORTED; a small
           first letter: RD_AROMATIC; ``@``s: RD_STEREO or RD_STEREO_DROPPED; anything else out of place, the end of the
           string included: RD_SYNTAX.  Counts saturate at 1000.  A token without an error bit is looked up: its symbol
           in the atom types (RD_ELEMENT), its charge in the charges (RD_CHARGE).
  C walk   only without an error bit so far; it ends at its first error.  One pass over the tokens with a branch stack
           of 128 entries and a ring table of 100: RD_SYNTAX (a bond or ring digit without an atom to its left, two
           bond symbols, ``(`` without an atom or behind a bond symbol or behind ``(``, ``)`` without ``(`` or behind a
           bond symbol or behind ``(``, a 129th open branch, ``.`` without an atom to its left or behind a bond symbol,
           ``%`` without two digits, an open branch or a dangling bond at the end), RD_RING_OPEN, RD_RING_ORDER,
           RD_SELF_LOOP, RD_MULTI_BOND, RD_BOND_ORDER; RD_FRAGMENTS (informational) from the components of the graph.
  D atoms  only without an error bit so far: x = the bond-order sum; a bare atom's hydrogens are the OpenSMILES
           implicit count (v - x, v the smallest normal valence >= x, 0 without one), a bracket atom's the stated
           ones; with an implicit-H segment the count is looked up (RD_HCOUNT); RD_OVER (informational) when x
           exceeds every allowed valence of the type and charge.
  out      with an error bit: the all-zero molecule, n_nodes 0 (RD_TOO_MANY: the need), atom_pos -1.  Otherwise node
           row i = one entry per segment (type | charge | implicit H if any | ``none_chirality`` inside what is left of
           the row, if anything is), edges symmetric and one-hot per bonded pair, atom_pos = the offset of the token."""
import numpy as np

RD_MULTI_BOND, RD_EMPTY, RD_SELF_LOOP, RD_OVER, RD_FRAGMENTS, RD_AROMATIC, RD_TOO_MANY = 16, 128, 256, 512, 1024, 2048, 16384
(RD_SYNTAX, RD_RING_OPEN, RD_RING_ORDER, RD_ELEMENT, RD_CHARGE, RD_HCOUNT, RD_BOND_ORDER, RD_STEREO, RD_STEREO_DROPPED,
 RD_UNSUPPORTED) = (1 << k for k in range(16, 26))
RD_INFO = RD_OVER | RD_FRAGMENTS | RD_STEREO_DROPPED
RD_ERROR = (RD_MULTI_BOND | RD_EMPTY | RD_SELF_LOOP | RD_AROMATIC | RD_TOO_MANY | RD_SYNTAX | RD_RING_OPEN |
            RD_RING_ORDER | RD_ELEMENT | RD_CHARGE | RD_HCOUNT | RD_BOND_ORDER | RD_STEREO | RD_UNSUPPORTED)
MAX_DEPTH, MAX_RINGS, SATURATE = 128, 100, 1000

NORMAL = {b"B": (3,), b"C": (4,), b"N": (3, 5), b"O": (2,), b"P": (3, 5), b"S": (2, 4, 6), b"F": (1,), b"I": (1,),
          b"Cl": (1,), b"Br": (1,)}
T_SKIP, T_ATOM, T_BOND1, T_BOND2, T_BOND3, T_DIGIT, T_PERCENT, T_OPEN, T_CLOSE, T_DOT = range(10)


def _digit(b):
    return 48 <= b <= 57


def _upper(b):
    return 65 <= b <= 90


def _lower(b):
    return 97 <= b <= 122


def classify(s, drop_stereo):
    """Stage A -> (class of every byte, flags, offsets of the atom tokens)."""
    cls, flags, starts, inside = [T_SKIP] * len(s), 0, [], False
    for k, b in enumerate(s):
        ch = chr(b)
        if ch == "[":
            if inside:
                flags |= RD_SYNTAX
            else:
                cls[k] = T_ATOM
                starts.append(k)
            inside = True
        elif ch == "]":
            if not inside:
                flags |= RD_SYNTAX
            inside = False
        elif inside:
            pass                                                            # stage B reads it
        elif ch in "BCNOPSFI":
            cls[k] = T_ATOM
            starts.append(k)
        elif (ch == "l" and k > 0 and s[k - 1] == ord("C")) or (ch == "r" and k > 0 and s[k - 1] == ord("B")):
            pass
        elif _upper(b):
            flags |= RD_SYNTAX
        elif ch in "bcnops" or ch == ":":
            flags |= RD_AROMATIC
        elif ch in "/\\":
            flags |= RD_STEREO_DROPPED if drop_stereo else RD_STEREO
            cls[k] = T_BOND1
        elif ch in "$*":
            flags |= RD_UNSUPPORTED
        elif ch in "-=#":
            cls[k] = {"-": T_BOND1, "=": T_BOND2, "#": T_BOND3}[ch]
        elif _digit(b):
            cls[k] = T_DIGIT
        elif ch in "%().":
            cls[k] = {"%": T_PERCENT, "(": T_OPEN, ")": T_CLOSE, ".": T_DOT}[ch]
        else:
            flags |= RD_SYNTAX
    return cls, flags, starts


def parse_atom(s, k, drop_stereo):
    """Stage B, the token at offset k -> (flags, symbol bytes, charge, stated hydrogens or None for a bare atom)."""
    def at(j):
        return s[j] if j < len(s) else 0

    if s[k] != ord("["):
        two = s[k:k + 2]
        return 0, two if two in (b"Cl", b"Br") else s[k:k + 1], 0, None
    j, flags = k + 1, 0
    if _digit(at(j)) or at(j) == ord("*"):
        return RD_UNSUPPORTED, b"", 0, 0
    if _lower(at(j)):
        return RD_AROMATIC, b"", 0, 0
    if not _upper(at(j)):
        return RD_SYNTAX, b"", 0, 0
    sym = bytes([at(j)])
    j += 1
    if _lower(at(j)):
        sym += bytes([at(j)])
        j += 1
    if at(j) == ord("@"):
        while at(j) == ord("@"):
            j += 1
        flags |= RD_STEREO_DROPPED if drop_stereo else RD_STEREO
    h = q = 0
    if at(j) == ord("H"):
        j, h = j + 1, 1
        if _digit(at(j)):
            h = 0
            while _digit(at(j)):
                h, j = min(h * 10 + at(j) - 48, SATURATE), j + 1
    if at(j) in (ord("+"), ord("-")):
        sign = at(j)
        j += 1
        if at(j) == sign:
            return flags | RD_UNSUPPORTED, sym, 0, h
        m = 1
        if _digit(at(j)):
            m = 0
            while _digit(at(j)):
                m, j = min(m * 10 + at(j) - 48, SATURATE), j + 1
        q = m if sign == ord("+") else -m
    if at(j) == ord(":"):
        flags |= RD_UNSUPPORTED
    elif at(j) != ord("]"):
        flags |= RD_SYNTAX
    return flags, sym, q, h


def read_one(row, length, rules, N, Fn, Fe, none_chirality=0, drop_stereo=False):
    """One string (``row``: max_len bytes; ``length`` or None) -> dict(nodes [N, Fn] int8, edges [N, N, Fe] int8,
    n_nodes, status, atom_pos [N] int32)."""
    A, C, H = rules.groups
    assert A + C + H <= Fn and (A + C + H == Fn or 0 <= none_chirality < Fn - (A + C + H)) and len(rules.order2) == Fe
    row = bytes(bytearray(np.asarray(row, np.uint8)))
    nodes, edges = np.zeros((N, Fn), np.int8), np.zeros((N, N, Fe), np.int8)
    pos = np.full(N, -1, np.int32)

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
    cls, status, starts = classify(s, drop_stereo)
    n = len(starts)
    if n > N:
        return result(status | RD_TOO_MANY, n)

    # B: the atom tokens
    a_idx, c_idx, stated = [0] * n, [0] * n, [None] * n
    symbols = [t.encode("ascii") for t in rules.atom_types]
    for i, k in enumerate(starts):
        flags, sym, q, stated[i] = parse_atom(s, k, drop_stereo)
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
    order = {}                                                              # (i, j), both ways -> the bond order
    root = list(range(n))

    def find(x):
        while root[x] != x:
            x = root[x]
        return x

    def bond(a, b, o):
        if a == b:
            return RD_SELF_LOOP
        if (a, b) in order:
            return RD_MULTI_BOND
        if 2 * o not in rules.order2:
            return RD_BOND_ORDER
        order[(a, b)] = order[(b, a)] = o
        ra, rb = find(a), find(b)
        root[max(ra, rb)] = min(ra, rb)
        return 0

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
                err = bond(prev, atoms, pending or 1)
            elif pending:
                err = RD_SYNTAX
            prev, pending, atoms = atoms, 0, atoms + 1
        elif t in (T_BOND1, T_BOND2, T_BOND3):
            if pending or prev < 0:
                err = RD_SYNTAX
            pending = {T_BOND1: 1, T_BOND2: 2, T_BOND3: 3}[t]
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
                        err = bond(other, prev, pending or o or 1)
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


def pack(strings, max_len=None):
    """Model of ``analyze.pack_strings`` on the host -> (text [G, max_len] uint8, length [G] int32)."""
    raw = [s.encode("ascii") if isinstance(s, str) else bytes(s) for s in strings]
    need = max([len(r) for r in raw] + [1])
    max_len = (need + 15) // 16 * 16 if max_len is None else max_len
    text = np.zeros((len(raw), max_len), np.uint8)
    for g, r in enumerate(raw):
        text[g, :len(r)] = np.frombuffer(r, np.uint8)
    return text, np.array([len(r) for r in raw], np.int32)


def read_batch(text, length, rules, N, Fn=None, Fe=None, none_chirality=0, drop_stereo=False):
    """Batch model of ``analyze.read_smiles`` -> dict(nodes [G, N, Fn] int8, edges [G, N, N, Fe] int8, n_nodes / status
    [G] int32, atom_pos [G, N] int32).  ``text``: [G, max_len] uint8 or a list of str (packed here, with lengths)."""
    if not isinstance(text, np.ndarray):
        text, length = pack(text)
    Fn = sum(rules.groups) if Fn is None else Fn
    Fe = len(rules.order2) if Fe is None else Fe
    G = len(text)
    out = dict(nodes=np.zeros((G, N, Fn), np.int8), edges=np.zeros((G, N, N, Fe), np.int8),
               n_nodes=np.zeros(G, np.int32), status=np.zeros(G, np.int32), atom_pos=np.full((G, N), -1, np.int32))
    for g in range(G):
        one = read_one(text[g], None if length is None else int(length[g]), rules, N, Fn, Fe, none_chirality,
                       drop_stereo)
        for name, value in one.items():
            out[name][g] = value
    return out
