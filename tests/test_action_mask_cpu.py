"""The action mask of constrained generation, model only (tests/action_mask_model.py is the specification the device
is held to in tests/test_action_mask_gpu.py): hand cases whose admissible set is written out here without the model,
the structural rules against the sampler model pinned to the reference's ``get_invalid_actions``, and closure — random
admissible action sequences from the empty graph end in valid, connected molecules within the action bound."""
import itertools

import numpy as np
import pytest

from oracle import sampler_oracle as SO
from tests import action_mask_model as AM
from tests import grow_oracle as GO
from tests import valence_model as VM

TYPES, CHARGES = ["C", "N", "O", "S", "Cl"], [-1, 0, 1]
# the largest allowed valence of every (type, charge), written out by hand from the table in tests/valence_model.py
VMAX = {"C": (3, 4, 3), "N": (2, 3, 4), "O": (1, 2, 3), "S": (1, 6, 5), "Cl": (0, 1, 6)}
IMP_H = [0, 1, 2, 3]


def rules_of(imp_h=None, bond_orders=(1, 2, 3)):
    return VM.Rules(TYPES, CHARGES, imp_H=imp_h, bond_orders=bond_orders)


def columns(dim_f_add, add, conn, term):
    """The admissible set as a bool [W] from hand-written predicates: ``add(i, type, charge, *rest, f)`` with the
    symbols and charges themselves, ``conn(i, f)``; the ravel is the reference's reshape of the APD row."""
    N, sub = dim_f_add[0], dim_f_add[1:]
    Fe = sub[-1]
    out = []
    for idx in itertools.product(*(range(d) for d in dim_f_add)):
        out.append(bool(add(idx[0], TYPES[idx[1]], idx[2], *idx[3:])))
    for i, f in itertools.product(range(N), range(Fe)):
        out.append(bool(conn(i, f)))
    out.append(bool(term))
    return np.array(out)


def vmax(sym, c):
    return VMAX[sym][c]                                       # c: the charge's index (0: -1, 1: 0, 2: +1)


def check(rules, dim_f_add, atoms, bonds, want, n=None, status=0, **kw):
    N = dim_f_add[0]
    nodes, edges = VM.molecule(N, rules, atoms, bonds, Fn=sum(dim_f_add[1:-1]), Fe=dim_f_add[-1])
    got, st = AM.admissible(nodes, edges, len(atoms) if n is None else n, rules, dim_f_add, **kw)
    assert st == status
    assert got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"columns {bad[:10]} differ: model {got[bad[:10]]}"
    return got


D3 = [5, 5, 3, 3]                                             # N = 5, W = 5 * 45 + 15 + 1
NO = lambda *a: False                                         # noqa: E731


def test_vmax_table_is_the_rules():
    assert {s: tuple(AM.vmax_table(rules_of())[k]) for k, s in enumerate(TYPES)} == VMAX


def test_empty_graph():
    want = columns(D3, lambda i, t, c, f: i == 0, NO, False)  # any atom (Cl- too: no bond is set), any f, at slot 0
    got = check(rules_of(), D3, [], [], want)
    assert got.sum() == 45 and got[:45].all()
    check(rules_of(), D3, [], [], columns(D3, lambda i, t, c, f: i == 0, NO, True), allow_empty=True)


def test_one_carbon():
    want = columns(D3, lambda i, t, c, f: i == 0 and f + 1 <= min(4, vmax(t, c)), NO, True)
    got = check(rules_of(), D3, [("C", 0)], [], want)
    assert got.sum() == 9 + 8 + 6 + 7 + 4 + 1                # per element: sum over charges of min(3, vmax); terminate


def test_saturated_carbon_takes_nothing():
    D = [6, 5, 3, 3]
    atoms = [("C", 0)] * 5
    bonds = [(0, k, 1) for k in range(1, 5)]
    want = columns(D, lambda i, t, c, f: 1 <= i <= 4 and f + 1 <= min(3, vmax(t, c)),
                   lambda i, f: 1 <= i <= 3, True)           # atom 0 is bonded to the last atom AND has no budget
    check(rules_of(), D, atoms, bonds, want)


def test_carbonyl_oxygen():
    want = columns(D3, lambda i, t, c, f: i == 0 and f + 1 <= min(2, vmax(t, c)), NO, True)
    check(rules_of(), D3, [("C", 0), ("O", 0)], [(0, 1, 2)], want)


def test_ammonium_with_four_bonds():
    D = [6, 5, 3, 3]
    atoms = [("N", 1)] + [("C", 0)] * 4
    want = columns(D, lambda i, t, c, f: 1 <= i <= 4 and f + 1 <= min(3, vmax(t, c)), lambda i, f: 1 <= i <= 3, True)
    check(rules_of(), D, atoms, [(0, k, 1) for k in range(1, 5)], want)


def test_oxide_and_chlorine_with_one_bond():
    for sym, ch in (("O", -1), ("Cl", 0)):
        want = columns(D3, lambda i, t, c, f: i == 0 and f + 1 <= min(3, vmax(t, c)), NO, True)
        check(rules_of(), D3, [("C", 0), (sym, ch)], [(0, 1, 1)], want)


def test_full_graph_and_bonded_pairs():
    D = [4, 5, 3, 3]
    atoms = [("C", 0)] * 4                                     # a chain 0-1-2-3: n == N, the last atom is bonded to 2
    want = columns(D, NO, lambda i, f: i == 0 or (i == 1 and f <= 1), True)      # atom 1 has 8 - 4 = 4 left
    check(rules_of(), D, atoms, [(0, 1, 1), (1, 2, 1), (2, 3, 1)], want)
    # 0=3 double as well: only 1 is left, and atom 3 has budget 8 - 2 - 4 = 2: a single bond
    want = columns(D, NO, lambda i, f: i == 1 and f == 0, True)
    check(rules_of(), D, atoms, [(0, 1, 1), (1, 2, 1), (2, 3, 1), (0, 3, 2)], want)


def test_implicit_h_segment():
    D = [5, 5, 3, 4, 3]
    rules = rules_of(IMP_H)
    # CH3-N(H1): C has 8 - 2 - 6 = 0 left, N 6 - 2 - 2 = 2; the new atom's own h counts against its valence
    want = columns(D, lambda i, t, c, h, f: i == 1 and f == 0 and 2 * (f + 1) + 2 * h <= 2 * vmax(t, c), NO, True)
    got = check(rules, D, [("C", 0, 3), ("N", 0, 1)], [(0, 1, 1)], want)
    assert got.sum() > 1
    # the empty graph: 2 h <= 2 vmax, any f
    want = columns(D, lambda i, t, c, h, f: i == 0 and h <= vmax(t, c), NO, False)
    check(rules, D, [], [], want)


def test_aromatic_bond_counts_three_halves():
    D = [5, 5, 3, 4]
    rules = rules_of(bond_orders=(1, 2, 3, 1.5))
    o2 = (2, 4, 6, 3)
    # C:N with one order-1.5 bond: N has 6 - 3 = 3 left (a single or an aromatic bond), C 8 - 3 = 5
    want = columns(D, lambda i, t, c, f: i <= 1 and o2[f] <= (5, 3)[i] and o2[f] <= 2 * vmax(t, c), NO, True)
    check(rules, D, [("C", 0), ("N", 0)], [(0, 1, 1.5)], want)


def test_chirality_group_is_ignored():
    D = [5, 5, 3, 4, 3, 3]
    rules = rules_of(IMP_H)
    N = D[0]
    nodes, edges = VM.molecule(N, rules, [("C", 0, 2), ("O", 0, 1)], [(0, 1, 1)], Fn=15, Fe=3)
    nodes[0, 12] = nodes[1, 14] = 1                           # a chirality entry per atom: not looked at
    got, st = AM.admissible(nodes, edges, 2, rules, D)
    want = columns(D, lambda i, t, c, h, x, f: (i == 0 and 2 * (f + 1) <= 2 and 2 * (f + 1) + 2 * h <= 2 * vmax(t, c)),
                   NO, True)                                  # C: 8 - 2 - 4 = 2, O: 4 - 2 - 2 = 0
    assert st == 0 and np.array_equal(got, want)
    add = got[:N * 5 * 3 * 4 * 3 * 3].reshape(N, 5, 3, 4, 3, 3)
    assert (add == add[:, :, :, :, :1, :]).all()


def test_states_that_are_not_well_formed_get_the_structural_rules_and_the_bit():
    rules = rules_of()
    s = GO.new_state(2, 5, 8, 3, 4, 4)                        # graph 0 of the reference's loop
    got, st = AM.admissible(s["nodes"][0], s["edges"][0], 1, rules, D3)
    assert st & AM.MASK_STRUCTURAL and st & VM.MOL_ONEHOT and st & VM.VAL_SELF_LOOP and st & VM.MOL_NODE_PAST_N
    assert np.array_equal(got, columns(D3, lambda i, t, c, f: i == 0, NO, True))
    # two bond types on one pair: over-valent adds are NOT masked, the bonded pair still is
    nodes, edges = VM.molecule(5, rules, [("O", 0), ("O", 0), ("C", 0)], [(0, 1, 1), (0, 1, 2), (1, 2, 1)])
    got, st = AM.admissible(nodes, edges, 3, rules, D3)
    assert st == VM.MOL_MULTI_BOND | AM.MASK_STRUCTURAL
    assert np.array_equal(got, columns(D3, lambda i, t, c, f: i <= 2, lambda i, f: i == 0, True))
    got, st = AM.admissible(nodes, edges, 3, rules, D3, valence=False)
    assert st == VM.MOL_MULTI_BOND | AM.MASK_STRUCTURAL


def random_walk(rng, rules, dim_f_add, steps):
    """A state reached from the empty graph by `steps` random admissible actions (stops at terminate)."""
    N, groups, Fe, A, W = AM.dims(dim_f_add)
    nodes, edges, n = np.zeros((N, sum(groups)), np.int8), np.zeros((N, N, Fe), np.int8), 0
    for _ in range(steps):
        ok, st = AM.admissible(nodes, edges, n, rules, dim_f_add)
        assert st == 0
        j = int(rng.choice(np.flatnonzero(ok[:-1]))) if ok[:-1].any() else W - 1
        if j == W - 1:
            break
        n = AM.apply_action(nodes, edges, n, j, dim_f_add)
    return nodes, edges, n


def test_structural_rules_are_the_samplers():
    """allow_empty, valence off: column j is admissible exactly when the sampler model (pinned to the reference's
    get_invalid_actions by tests/test_sampler_cpu.py) does not flag the forced draw of j."""
    rules, D = rules_of(), [4, 5, 3, 3]
    N, groups, Fe, A, W = AM.dims(D)
    rng = np.random.default_rng(5)
    states = [random_walk(rng, rules, D, k) for k in (0, 1, 2, 3, 4, 5, 6, 8, 10, 12)]
    states.append((*VM.molecule(N, rules, [("C", 0)] * 4, [(0, 1, 1), (1, 2, 2), (2, 3, 1)]), 4))
    assert any(n == N for _, _, n in states) and any(n == 0 for _, _, n in states)
    apds = np.full((W, W), 1.0 / W)
    for nodes, edges, n in states:
        got, st = AM.admissible(nodes, edges, n, rules, D, allow_empty=True, valence=False)
        assert st == 0
        out = SO.get_actions(apds, np.arange(W), np.full(W, n, np.int64), np.broadcast_to(edges, (W, N, N, Fe)),
                             D, [N, Fe])
        flagged = np.zeros(W, bool)
        flagged[out["invalid"]] = True
        assert np.array_equal(got, ~flagged), (n, np.flatnonzero(got == flagged)[:8])


def test_closure_random_admissible_sequences_end_valid_connected_and_bounded():
    """2000 molecules grown by uniformly random admissible actions through the numpy growth model
    (tests/grow_oracle.grow_round), N = 13: each is valid under tests/valence_model.py, connected, and took no more
    actions than ``n + sum vmax / 2 - (n - 1) + 1``."""
    rules, D = rules_of(), [13, 5, 3, 3]
    N, groups, Fe, A, W = AM.dims(D)
    B, want = 401, 2000
    vm = AM.vmax_table(rules)
    bound_all = AM.action_bound(N, N * int(vm.max()))
    s = GO.new_state(B, N, sum(groups), Fe, 4096, want + B)
    s["target"] = want
    rng = np.random.default_rng(11)
    while s["n"] < want:
        action = np.zeros((B, 4), np.int32)
        for b in range(B):
            n = int(s["n_nodes"][b])
            ok, st = AM.admissible(s["nodes"][b], s["edges"][b], n, rules, D)
            assert (st == 0) == (b != 0)
            pick = np.flatnonzero(ok[:-1]) if b == 0 else np.flatnonzero(ok)      # graph 0 never terminates here
            j = int(rng.choice(pick))
            if j == W - 1:
                action[b] = (2, 0, 0, 0)
            elif j < N * A:
                action[b] = (0, j // A, j % A, 0 if n == 0 else n)
            else:
                action[b] = (1, (j - N * A) // Fe, (j - N * A) % Fe, n - 1)
        GO.grow_round(s, action, np.ones(B, np.float32), np.zeros(B, np.int32), groups, Fe)
        assert s["error"] == 0 and s["round"] < 4000
    G = s["n"]
    assert G >= want and s["properly_terminated"][:G].all()
    nn = s["generated_n_nodes"][:G].astype(np.int64)
    out = VM.validity(s["generated_nodes"][:G], s["generated_edges"][:G], nn, rules, require_connected=True)
    assert (out["valid"] == 1).all() and (out["desc"][:, 4] == 1).all()
    assert not (out["status"] & (VM.VAL_OVER | VM.VAL_FRAGMENTS | VM.VAL_SELF_LOOP | VM.MALFORMED)).any()
    n_actions = (s["generated_likelihoods"][:G] != 0).sum(axis=1)
    types = s["generated_nodes"][:G, :, :5].argmax(-1)
    charges = s["generated_nodes"][:G, :, 5:8].argmax(-1)
    live = np.arange(N)[None] < nn[:, None]
    vsum = (vm[types, charges] * live).sum(axis=1)
    bound = np.array([AM.action_bound(int(n), int(v)) for n, v in zip(nn, vsum)])
    assert (n_actions <= bound).all() and bound.max() <= bound_all
    assert n_actions.max() > 2 and nn.max() == N               # the walk reaches full graphs


def test_pack_bits_layout():
    a = np.zeros((2, 70), bool)
    a[0, [0, 31, 32, 69]] = True
    w = AM.pack_bits(a)
    assert w.shape == (2, 3) and w.dtype == np.uint32
    assert list(w[0]) == [1 | (1 << 31), 1, 1 << 5] and not w[1].any()
