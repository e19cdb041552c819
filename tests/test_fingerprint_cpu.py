"""CPU: the numpy specification of molecule scoring (tests/fingerprint_model.py) pinned independently, the golden, the
binding and the Python boundary of graphinvent_amd.analyze.fingerprint / FingerprintSet / similarity / KernelModel /
activity / target_size_score / compute_score.  No device compute is issued.

The fingerprint is a Morgan-style fingerprint of the labelled graph, NOT RDKit's ECFP bits; what pins it here is
networkx's Weisfeiler-Lehman hashes (the partition of all atoms of a set by id_r, r = 0 .. 3), node-order invariance,
hand-checked molecules, and scikit-learn's own decision_function / predict_proba of two fitted SVCs
(tests/golden/golden_fingerprint.npz, made by tests/golden/make_golden_fingerprint.py)."""
import os
import re

import numpy as np
import pytest
import torch

from graphinvent_amd import analyze
from graphinvent_amd import lib as L
from tests import canon_model as CM
from tests import fingerprint_model as FM
from tests import valence_model as VM
from tests.test_valence_cpu import RULE_ARGS, model_rules, shipped, status_cases, stored_set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = ("gdb13", "arom5", "chiral6", "atoms_charges", "imp_h_chirality")
_CACHE = {}


def golden(golden_dir):
    if "golden" not in _CACHE:
        _CACHE["golden"] = np.load(os.path.join(golden_dir, "golden_fingerprint.npz"))
    return _CACHE["golden"]


def set_of(golden_dir, c):
    """(nodes, edges, n_nodes or None, rules name) of a stored set or of the 30 shipped molecules."""
    if c == "shipped":
        nodes, edges, _ = shipped(golden_dir)
        return nodes, edges, None, "gdb13"
    nodes, edges, n, _ = stored_set(golden_dir, c)
    return nodes, edges, n, c


def model_fp(golden_dir, c, radius=2, n_bits=2048):
    """The model's fingerprints of set c, computed once per (radius, n_bits) and shared (read only)."""
    key = ("fp", c, radius, n_bits)
    if key not in _CACHE:
        nodes, edges, n, r = set_of(golden_dir, c)
        _CACHE[key] = FM.fingerprint(nodes, edges, n, model_rules(r), radius=radius, n_bits=n_bits)
    return _CACHE[key]


def hand(atoms, bonds, N=6):
    return VM.molecule(N, model_rules("gdb13"), atoms, bonds)


def fp_one(nodes, edges, n=None, radius=2, n_bits=2048, rules="gdb13"):
    out = FM.fingerprint(nodes[None], edges[None], None if n is None else [n], model_rules(rules), radius, n_bits)
    return {k: v[0] for k, v in out.items()}


# ---- the fingerprint model -------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", SETS + ("shipped",))
def test_model_partitions_atoms_as_networkx_wl_does(golden_dir, c):
    D = golden(golden_dir)
    assert c in D["wl::sets"]
    fp = model_fp(golden_dir, c, radius=3, n_bits=64)
    mol, atom, classes = D[f"wl::{c}::mol"], D[f"wl::{c}::atom"], D[f"wl::{c}::classes"]
    live = [g for g in range(len(fp["ids"])) if fp["ids"][g] is not None]
    assert sorted(set(mol.tolist())) == live and len(mol) == sum(fp["ids"][g].shape[1] for g in live) > 50
    for r in range(4):
        ids = [int(fp["ids"][g][r, i]) for g, i in zip(mol.tolist(), atom.tolist())]
        to_class, to_id = {}, {}
        for x, k in zip(ids, classes[:, r].tolist()):                    # both directions: a bijection
            assert to_class.setdefault(x, k) == k and to_id.setdefault(k, x) == x, (c, r)
        assert len(to_class) == classes[:, r].max() + 1
    assert classes[:, 3].max() >= classes[:, 0].max()                    # refinement only splits


@pytest.mark.parametrize("c", SETS)
def test_node_order_does_not_matter(golden_dir, c):
    nodes, edges, n_nodes, r = set_of(golden_dir, c)
    want = model_fp(golden_dir, c, radius=2, n_bits=256)
    rng = np.random.default_rng(5)
    tried = 0
    for g in range(len(nodes)):
        if want["ids"][g] is None:
            continue
        n = want["ids"][g].shape[1]
        pn, pe, perms = [], [], []
        for _ in range(8):
            perms.append(rng.permutation(n))
            a, b = CM.permute(nodes[g], edges[g], perms[-1])
            pn.append(a); pe.append(b)
        got = FM.fingerprint(np.stack(pn), np.stack(pe), None if n_nodes is None else [n] * 8, model_rules(r), 2, 256)
        for k, perm in enumerate(perms):
            assert got["status"][k] == 0 and got["popcount"][k] == want["popcount"][g]
            assert np.array_equal(got["bits"][k], want["bits"][g]), (c, g, k)
            assert np.array_equal(got["atom_id"][k, :n], want["atom_id"][g, perm]), (c, g, k)
            assert (got["atom_id"][k, n:] == -1).all()
        tried += 1
    assert tried >= 10


def test_isomorphic_molecules_get_equal_rows(golden_dir):
    src_n, src_e, _, _ = set_of(golden_dir, "gdb13")
    C = np.load(os.path.join(golden_dir, "golden_canon.npz"))             # a batch with planted, permuted duplicates
    mols = [CM.permute(src_n[m], src_e[m], p[:CM.derived_n(src_n[m])]) for m, p in zip(C["mix::src"], C["mix::perm"])]
    nodes, edges = np.stack([a for a, _ in mols]), np.stack([b for _, b in mols])
    uniq, rep, counts = CM.unique(CM.canonical(nodes, edges))
    fp = FM.fingerprint(nodes, edges, None, model_rules("gdb13"))
    assert 0 < (uniq == 0).sum() and counts[2] < len(nodes)               # the batch holds duplicates to find
    for g in np.flatnonzero(rep != np.arange(len(nodes))):
        assert np.array_equal(fp["bits"][g], fp["bits"][rep[g]]) and fp["popcount"][g] == fp["popcount"][rep[g]]
    distinct = {fp["bits"][g].tobytes() for g in np.flatnonzero(rep == np.arange(len(nodes)))}
    assert len(distinct) > 0.9 * counts[2]                                # and different molecules mostly differ


def test_hand_checked_molecules():
    for R in range(FM.MAX_RADIUS + 1):
        methane = fp_one(*hand([("C", 0)], []), radius=R)
        assert methane["status"] == 0 and 1 <= methane["popcount"] <= R + 1
        ring = fp_one(*hand([("C", 0)] * 6, [(i, (i + 1) % 6, 1) for i in range(6)]), radius=R)
        assert ring["status"] == 0 and 1 <= ring["popcount"] <= R + 1     # one identifier per radius
        assert len({int(x) for x in ring["ids"][R]}) == 1 and ring["ids"].shape == (R + 1, 6)
    ethane, ethene = fp_one(*hand([("C", 0)] * 2, [(0, 1, 1)])), fp_one(*hand([("C", 0)] * 2, [(0, 1, 2)]))
    assert not np.array_equal(ethane["bits"], ethene["bits"]) and ethane["popcount"] <= 3
    assert ethane["ids"][0, 0] == ethane["ids"][0, 1] != ethene["ids"][0, 0]
    # id_0 by hand: carbon (a 0), neutral (c 1 of [-1, 0, 1]), one partner, a single bond (o2 2)
    assert int(ethane["ids"][0, 0]) == CM.mix64((int(FM.K0) + 0 + 256 * 1 + (1 << 16) + (2 << 24)) & CM.MASK)
    acid = hand([("C", 0), ("C", 0), ("O", 0), ("O", 0), ("N", 1)], [(0, 1, 1), (1, 2, 2), (1, 3, 1), (0, 4, 1)])
    zero = fp_one(*acid, radius=0, n_bits=4096)
    assert np.array_equal(zero["bits"], FM.fold(zero["ids"][0], 4096)) and zero["ids"].shape == (1, 5)
    two = fp_one(*acid, radius=2, n_bits=4096)
    assert np.array_equal(two["ids"][0], zero["ids"][0]) and two["popcount"] > zero["popcount"]
    # id_1 of the carbonyl oxygen by hand: itself, and its one neighbour through a double bond (order2 4)
    k1x4 = (int(FM.K1) * 4) & CM.MASK
    want = CM.mix64((CM.mix64((int(two["ids"][0, 2]) + 1) & CM.MASK) + CM.mix64(int(two["ids"][0, 1]) ^ k1x4)) & CM.MASK)
    assert int(two["ids"][1, 2]) == want
    small = fp_one(*acid, radius=2, n_bits=64)                            # 64 bits: the OR of the 64-bit slices
    wide = two["bits"].view(np.uint32).reshape(64, 2)
    assert np.array_equal(small["bits"].view(np.uint32), np.bitwise_or.reduce(wide, axis=0))
    assert small["popcount"] <= two["popcount"] == len({int(x) & 4095 for x in two["ids"].reshape(-1)})
    assert FM.valid_n_bits(64) and FM.valid_n_bits(4096) and not any(FM.valid_n_bits(b) for b in (32, 96, 8192, 2048.0))


def test_status_and_zero_rows():
    cases = status_cases()
    r = model_rules("gdb13")
    for name, (nodes, edges, n, valence_status) in cases.items():
        want = valence_status & FM.ZERO_ROW                               # OVER / FRAGMENTS are not the fingerprint's
        for given in (n, None) if name not in ("n_too_large", "onehot_none") else (n,):
            got = FM.fingerprint(nodes[None], edges[None], None if given is None else [given], r)
            assert got["status"][0] == want, (name, given, got["status"][0])
            if want:
                assert not got["bits"].any() and got["popcount"][0] == 0 and (got["atom_id"] == -1).all(), name
                assert got["ids"][0] is None
            else:
                assert got["popcount"][0] > 0 and (got["atom_id"][0, 3:] == -1).all(), name
    seen = 0
    for name, (_, _, _, s) in cases.items():
        seen |= s
    assert seen & FM.ZERO_ROW == FM.ZERO_ROW                              # every bit that zeroes a row has its molecule
    assert {"sound", "over", "fragments"} == {k for k, c in cases.items() if not c[3] & FM.ZERO_ROW}


# ---- the comparison model --------------------------------------------------------------------------------------

def random_rows(rng, R, n_bits, density=0.1):
    return FM.pack(rng.random((R, n_bits)) < density)


def test_compare_model_against_a_dense_computation():
    rng = np.random.default_rng(11)
    for n_bits, G, S in ((64, 9, 40), (256, 12, 70), (2048, 5, 33)):
        q, s = random_rows(rng, G, n_bits), random_rows(rng, S, n_bits, 0.2)
        q[1] = 0                                                          # an empty query
        s[3] = 0                                                          # an empty set row
        q[2] = s[7]                                                       # a query that is in the set ...
        s[20] = s[7]                                                      # ... twice: the lower index wins
        s[5], s[6] = s[4], s[4]
        assert np.array_equal(FM.pack(FM.unpack(q)), q)
        Q, X = FM.unpack(q).astype(np.float64), FM.unpack(s).astype(np.float64)
        c = Q @ X.T
        a, b = Q.sum(axis=1), X.sum(axis=1)
        u = a[:, None] + b[None, :] - c
        sim = np.where(u > 0, c / np.maximum(u, 1), 0.0)
        w = rng.standard_normal(S)
        for kind, K in (("tanimoto", sim), ("rbf", np.exp(-0.03 * ((Q[:, None, :] - X[None, :, :]) ** 2).sum(axis=2))),
                        ("linear", c)):
            got = FM.compare(q, s, weight=w, kind=kind, gamma=0.03, intercept=0.25, prob_a=-1.5, prob_b=0.2)
            f = 0.25 + K @ w
            assert np.allclose(got["decision"], f, rtol=1e-12, atol=1e-12), kind
            with np.errstate(over="ignore"):                              # exp -> inf is 1 / inf = 0, as wanted
                p = 1.0 / (1.0 + np.exp(-1.5 * f + 0.2))
            p[1] = 0.0
            assert np.allclose(got["proba"], p, rtol=1e-12, atol=1e-15) and got["proba"][1] == 0.0, kind
            assert np.allclose(got["abs_sum"], 0.25 + np.abs(K * w).sum(axis=1), rtol=1e-12)
        best = np.argmax(sim, axis=1)                                     # the first maximum: the lowest index
        best[1] = -1
        assert np.array_equal(got["nearest"], best) and got["nearest"][2] == 7
        assert got["max_sim"][2] == 1.0 and got["common"][2] == got["union"][2] == int(a[2])
        assert got["nearest"][1] == -1 and got["max_sim"][1] == 0 and got["common"][1] == got["union"][1] == 0
        live = best >= 0
        assert np.array_equal(got["common"][live], c[live, best[live]].astype(np.int32))
        assert np.array_equal(got["union"][live], u[live, best[live]].astype(np.int32))
        assert np.array_equal(got["max_sim"][live], (c[live, best[live]].astype(np.float32)
                                                      / u[live, best[live]].astype(np.float32)))
        plain = FM.compare(q, s)
        assert "decision" not in plain and np.array_equal(plain["nearest"], got["nearest"])
    tie_q, tie_s = FM.pack(np.eye(64)[[0]]), FM.pack(np.concatenate([np.eye(64)[[1, 0, 0]], np.ones((1, 64))]))
    assert FM.compare(tie_q, tie_s)["nearest"][0] == 1                    # 0, 1, 1, 1 / 64: the first of the two ones
    assert FM.internal_diversity(tie_s[1:3]) == 0.0 and FM.internal_diversity(tie_s[:1]) == 0.0
    assert FM.internal_diversity(FM.pack(np.eye(64)[:5])) == 1.0
    assert abs(FM.internal_diversity(tie_s) - (1.0 - (2 * 1.0 + 6 / 64) / 12)) < 1e-15


@pytest.mark.parametrize("kind", ["rbf", "tanimoto"])
def test_model_decision_and_proba_against_sklearn(golden_dir, kind):
    D = golden(golden_dir)
    assert str(D["svc::train"]) == str(D["svc::test"]) == "gdb13"
    fp = model_fp(golden_dir, "gdb13", radius=int(D["svc::radius"]), n_bits=int(D["svc::n_bits"]))
    q = fp["bits"][D["svc::test_rows"]]
    f, p = D[f"svc::{kind}::decision"], D[f"svc::{kind}::proba"]
    gap = float(D[f"svc::{kind}::platt_gap"])
    got = FM.compare(q, D[f"svc::{kind}::support"], weight=D[f"svc::{kind}::dual_coef"], kind=kind,
                     gamma=float(D[f"svc::{kind}::gamma"]), intercept=float(D[f"svc::{kind}::intercept"]),
                     prob_a=float(D[f"svc::{kind}::probA"]),
                     prob_b=float(D[f"svc::{kind}::platt_sign"]) * float(D[f"svc::{kind}::probB"]))
    assert np.abs(got["decision"] - f).max() <= 1e-9 * np.abs(f).max()
    assert np.abs(got["proba"] - p).max() <= gap + 1e-12
    assert (p > 0.5).any() and (p < 0.5).any() and float(D[f"svc::{kind}::platt_sign"]) == -1.0
    assert 1e-6 < gap < 0.005          # libsvm's two-class probability is an iteration stopped at 0.0025, not the sigmoid
    if kind == "tanimoto":                                                # the support rows are training fingerprints
        train = fp["bits"][D["svc::train_rows"]]
        assert {r.tobytes() for r in D["svc::tanimoto::support"]} <= {r.tobytes() for r in train}


class _FittedSVC:
    """What KernelModel.from_sklearn reads of a fitted sklearn.svm.SVC, filled from the golden."""

    def __init__(self, D, kind, train_bits):
        self.kernel = "rbf" if kind == "rbf" else "precomputed"
        self.dual_coef_ = D[f"svc::{kind}::dual_coef"][None]
        self.intercept_ = np.array([float(D[f"svc::{kind}::intercept"])])
        self._gamma = float(D[f"svc::{kind}::gamma"])
        self.probA_, self.probB_ = np.array([float(D[f"svc::{kind}::probA"])]), np.array([float(D[f"svc::{kind}::probB"])])
        support = D[f"svc::{kind}::support"]
        if kind == "rbf":
            self.support_vectors_ = FM.unpack(support).astype(np.float64)
        else:                                                             # indices into the training rows
            index = {r.tobytes(): k for k, r in reversed(list(enumerate(train_bits)))}
            self.support_ = np.array([index[r.tobytes()] for r in support], np.int32)


def fitted_svc(golden_dir, kind):
    D = golden(golden_dir)
    fp = model_fp(golden_dir, "gdb13", radius=int(D["svc::radius"]), n_bits=int(D["svc::n_bits"]))
    train = fp["bits"][D["svc::train_rows"]]
    return _FittedSVC(D, kind, train), train


# ---- the scores ------------------------------------------------------------------------------------------------

def test_scores_equal_the_reference_outputs(golden_dir):
    D = golden(golden_dir)
    names = [str(n) for n in D["score::names"]]
    assert len(names) == 9 and {"single", "continuous", "binary", "zeros_uniqueness", "zeros_validity",
                                "zeros_termination"} <= set(names)
    for name in names:
        get = lambda k: D[f"score::{name}::{k}"]
        targets, N, score_type = get("targets").tolist(), int(get("max_n_nodes")), str(get("score_type"))
        thresholds = get("thresholds").tolist()
        n_nodes = torch.from_numpy(get("n_nodes"))
        masks = {k: torch.from_numpy(get(k)) for k in ("uniqueness", "validity", "termination")}
        contributions = [analyze.target_size_score(n_nodes, t, N) for t in targets]
        for k, c in enumerate(contributions):
            assert c.dtype == torch.float32 and torch.equal(c, torch.from_numpy(get("contributions")[k])), (name, k)
            assert np.array_equal(FM.target_size_score(get("n_nodes"), targets[k], N), get("contributions")[k])
        kept = [c.clone() for c in contributions]
        final = analyze.compute_score(contributions, score_type=score_type, thresholds=thresholds, **masks)
        assert final.dtype == torch.float32 and torch.equal(final, torch.from_numpy(get("final"))), name
        assert all(torch.equal(a, b) for a, b in zip(kept, contributions))           # the caller's tensors are kept
        model = FM.compute_score(get("contributions"), score_type, thresholds, get("uniqueness"), get("validity"),
                                 get("termination"))
        assert np.array_equal(model, get("final")), name
    assert np.array_equal(D["score::single::final"], D["score::single_ignores_binary::final"])       # the quirk
    assert set(np.unique(D["score::binary::final"]).tolist()) == {0.0, 1.0}
    for k in ("uniqueness", "validity", "termination"):
        mask, final = D[f"score::zeros_{k}::{k}"], D[f"score::zeros_{k}::final"]
        assert (mask == 0).any() and not final[mask == 0].any()
    one = torch.ones(3)
    with pytest.raises(NotImplementedError):
        analyze.compute_score([one, one], score_type="ranked", thresholds=[0, 0], uniqueness=one, validity=one,
                              termination=one)
    with pytest.raises(ValueError, match="do not match"):
        analyze.compute_score([one, one], score_type="binary", thresholds=[0], uniqueness=one, validity=one,
                              termination=one)
    with pytest.raises(ValueError, match="target"):
        analyze.target_size_score(one, 0, 13)
    with pytest.raises(ValueError, match="target"):
        analyze.target_size_score(one, 14, 13)


# ---- binding and boundary --------------------------------------------------------------------------------------

def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "graphinvent_amd.h")).read()
    lib = L.load()
    for name, n_args in (("gi_mol_fingerprint", 20), ("gi_fp_compare", 19)):
        assert re.search(rf"^int\s+{name}\s*\(", hdr, flags=re.M)
        assert name in L.SIGNATURES and hasattr(lib, name)
        decl = re.search(rf"^int\s+{name}\s*\((.*?)\);", hdr, flags=re.M | re.S).group(1)
        assert len(L.SIGNATURES[name][1]) == len(decl.split(",")) == n_args
    for name, value in (("MIN_BITS", 64), ("MAX_BITS", 4096), ("MAX_RADIUS", 4), ("TANIMOTO", 0), ("RBF", 1),
                        ("LINEAR", 2)):
        assert re.search(rf"#define\s+GI_FP_{name}\s+{value}\b", hdr) and getattr(L, "FP_" + name) == value
    assert (FM.TANIMOTO, FM.RBF, FM.LINEAR, FM.MAX_RADIUS) == (L.FP_TANIMOTO, L.FP_RBF, L.FP_LINEAR, L.FP_MAX_RADIUS)
    assert FM.ZERO_ROW == analyze.MALFORMED_BITS | L.VAL_EMPTY | L.VAL_SELF_LOOP
    assert lib.gi_abi_version() == L.ABI_VERSION                          # an added entry point is compatible
    src = open(os.path.join(ROOT, "graphinvent_amd", "csrc", "gi_fingerprint.hip")).read()
    assert "gi_fingerprint.hip" in open(os.path.join(ROOT, "graphinvent_amd", "csrc", "Makefile")).read()
    assert "getenv" not in src and "atomicAdd(&out" not in src
    assert f"0x{int(FM.K0):016X}ull" in src and f"0x{int(FM.K1):016X}ull" in src      # the kernel copies the constants
    assert int(FM.K0) & 1 and int(FM.K1) & 1
    assert "gi_mol_fingerprint" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    # argument checks that need no device: nothing is launched, nothing is written, for any of these
    def fp(G=0, N=13, Fn=8, Fe=3, dtype=0, nb=1, A=5, C=3, H=0, radius=2, n_bits=2048):
        return lib.gi_mol_fingerprint(G, N, Fn, Fe, None, None, dtype, None, nb, A, C, H, None, radius, n_bits, None,
                                      None, None, None, None)
    assert fp() == 0 and fp(radius=0) == 0 and fp(radius=4) == 0 and fp(n_bits=64) == 0 and fp(n_bits=4096) == 0
    assert fp(G=1) == -1                                                   # no buffers
    assert fp(radius=5) == -1 and fp(radius=-1) == -1
    assert [fp(n_bits=b) for b in (96, 32, 8192, 0, -64, 2047)] == [-1] * 6
    assert fp(N=129) == -1 and fp(N=0) == -1 and fp(Fe=9) == -1 and fp(G=-1) == -1 and fp(Fn=513) == -2
    assert fp(dtype=2) == -1 and fp(nb=2) == -1 and fp(A=6) == -1 and fp(H=1) == -1 and fp(A=0) == -1
    def cmp(G=0, S=1, Wq=64, Ws=64, kind=0):
        return lib.gi_fp_compare(G, S, Wq, Ws, None, None, None, kind, 0.0, 0.0, 0.0, 0.0, None, None, None, None, None,
                                 None, None)
    assert cmp() == 0 and cmp(Wq=2, Ws=2) == 0 and cmp(Wq=128, Ws=128) == 0 and cmp(kind=2) == 0
    assert cmp(G=1) == -1                                                  # no buffers
    assert cmp(S=0) == -1 and cmp(S=-3) == -1 and cmp(Wq=64, Ws=32) == -1 and cmp(Wq=3, Ws=3) == -1
    assert cmp(Wq=1, Ws=1) == -1 and cmp(Wq=256, Ws=256) == -1 and cmp(kind=3) == -1 and cmp(G=-1) == -1
    assert analyze.Fingerprints.nbytes(3, 5, 2, False) == 24 + 12 + 12
    assert analyze.Fingerprints.nbytes(3, 5, 2, True) == 48 + 120 and analyze.SetComparison.nbytes(3, True) == 72
    assert analyze.Fingerprints.layout(3, 5, 2, True)["bits"][0] == 0      # the rows lead: 16-byte aligned


def test_python_boundary_raises(golden_dir):
    n, e = torch.zeros(2, 13, 8, dtype=torch.int8), torch.zeros(2, 13, 13, 3, dtype=torch.int8)
    host_rules = analyze.ValenceRules(device=None, **RULE_ARGS["gdb13"])
    with pytest.raises(RuntimeError, match="no CPU"):                      # CPU tensors
        analyze.fingerprint(n, e, None, host_rules)
    with pytest.raises(TypeError, match="ValenceRules"):
        analyze.fingerprint(n, e, None, [5, 3])
    with pytest.raises(TypeError, match="tensor"):
        analyze.fingerprint(n.numpy(), e.numpy(), None, host_rules)
    for bad in (96, 32, 8192, 2048.0, True):
        with pytest.raises(ValueError, match="n_bits"):
            analyze.fingerprint(n, e, None, host_rules, n_bits=bad)
    for bad in (5, -1, 1.0):
        with pytest.raises(ValueError, match="radius"):
            analyze.fingerprint(n, e, None, host_rules, radius=bad)
    with pytest.raises(RuntimeError, match="no CPU"):
        analyze.FingerprintSet(np.zeros((3, 64), np.int32), device="cpu")
    with pytest.raises(ValueError, match="n_bits"):
        analyze.FingerprintSet(np.zeros((3, 96), np.uint8))
    with pytest.raises(ValueError, match="n_bits"):
        analyze.FingerprintSet(np.zeros((3, 3), np.int32))
    with pytest.raises(ValueError, match="only 0 and 1"):
        analyze.FingerprintSet(np.full((3, 64), 2, np.uint8))
    with pytest.raises(ValueError, match="at least one row"):
        analyze.FingerprintSet(np.zeros((0, 64), np.int32))
    with pytest.raises(TypeError, match="FingerprintSet"):
        analyze.KernelModel(np.zeros((3, 64), np.int32), [1, 2, 3], 0.0)
    with pytest.raises(TypeError, match="FingerprintSet"):
        analyze.similarity(torch.zeros(2, 2, dtype=torch.int32), np.zeros((3, 2), np.int32))
    with pytest.raises(TypeError, match="KernelModel"):
        analyze.activity(torch.zeros(2, 2, dtype=torch.int32), None)
    packed = analyze._pack_bits("t", np.eye(64, dtype=np.float32)[:3])     # any dtype but int32 is a 0 / 1 array
    assert packed.dtype == torch.int32 and np.array_equal(packed.numpy(), FM.pack(np.eye(64)[:3]))
    assert analyze._pack_bits("t", FM.pack(np.eye(64)[:3])).shape == (3, 2)           # int32 is packed already
    if not torch.cuda.is_available():
        return
    dn, de = n.cuda(), e.cuda()                                            # raised before anything is launched
    rules = analyze.ValenceRules(**RULE_ARGS["gdb13"])
    with pytest.raises(RuntimeError, match="device=None"):
        analyze.fingerprint(dn, de, None, host_rules)
    with pytest.raises(TypeError, match="float32 or both int8"):
        analyze.fingerprint(dn.float(), de, None, rules)
    with pytest.raises(TypeError, match="float32 or both int8"):
        analyze.fingerprint(dn.short(), de.short(), None, rules)
    with pytest.raises(TypeError, match="n_nodes"):
        analyze.fingerprint(dn, de, torch.zeros(2, device="cuda"), rules)
    with pytest.raises(ValueError, match="do not fit"):
        analyze.fingerprint(dn[:, :, :7].contiguous(), de, None, rules)
    with pytest.raises(ValueError, match="bond_orders is required"):
        analyze.fingerprint(dn, de[..., :2].contiguous(), None, rules)
    ref = analyze.FingerprintSet(np.zeros((3, 64), np.uint8))
    with pytest.raises(ValueError, match="128 bits, the set 64"):
        analyze.similarity(torch.zeros(2, 4, dtype=torch.int32, device="cuda"), ref)
    with pytest.raises(RuntimeError, match="no CPU"):
        analyze.similarity(torch.zeros(2, 2, dtype=torch.int32), ref)
    with pytest.raises(TypeError, match="packed int32"):
        analyze.similarity(torch.zeros(2, 2, device="cuda"), ref)
    with pytest.raises(ValueError, match="3 support rows"):
        analyze.KernelModel(ref, [1.0, 2.0], 0.0)
    with pytest.raises(ValueError, match="kind"):
        analyze.KernelModel(ref, [1.0, 2.0, 3.0], 0.0, kind="poly")
    with pytest.raises(ValueError, match="gamma"):
        analyze.KernelModel(ref, [1.0, 2.0, 3.0], 0.0, kind="rbf")
    with pytest.raises(ValueError, match="both prob_a and prob_b"):
        analyze.KernelModel(ref, [1.0, 2.0, 3.0], 0.0, prob_a=1.0)
    svc, train = fitted_svc(golden_dir, "tanimoto")
    with pytest.raises(ValueError, match="support_bits"):
        analyze.KernelModel.from_sklearn(svc)
    svc.dual_coef_ = np.zeros((2, 5))
    with pytest.raises(ValueError, match="two-class"):
        analyze.KernelModel.from_sklearn(svc, train)
