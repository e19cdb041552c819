"""Molecule log-likelihoods without a GPU: the torch restatement tests/likelihood_model.py on the oracle's logits
against golden_likelihood.npz (the unmodified reference model and ``Analyzer.get_validation_likelihood``;
tests/golden/make_golden_likelihood.py), the new C ABI symbols (declared, exported, bound; ABI version unchanged), and
graphinvent_amd.likelihood refusing CPU tensors."""
import os
import re

import numpy as np
import pytest
import torch

from graphinvent_amd import lib as L
from oracle import ggnn_oracle as O
from tests import likelihood_model as LM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gi_row_loglik", "gi_row_loglik_bwd", "gi_mol_loglik_sum", "gi_route_rows_hot")
#: test_oracle_golden.py's bar on the oracle's logits against the reference's, relative to the largest magnitude
ORACLE_LOGITS_BAR = 2e-6

_CACHE = {}


def golden():
    if "G" not in _CACHE:
        _CACHE["G"] = dict(np.load(os.path.join(GOLDEN, "golden_likelihood.npz")))
    return _CACHE["G"]


def route_set(name="gdb13::"):
    """(rows_nodes, rows_edges, hot, row_mol, mol_nodes, mol_edges, dim_f_add, dim_f_conn) of a golden_routes set."""
    if name not in _CACHE:
        R = np.load(os.path.join(GOLDEN, "golden_routes.npz"))
        _CACHE[name] = tuple(R[name + k] for k in ("rows_nodes", "rows_edges", "hot", "row_mol", "mol_nodes",
                                                   "mol_edges", "dim_f_add", "dim_f_conn"))
    return _CACHE[name]


def golden_weights():
    """(cfg, state dict) of the trained small model (golden_generator.npz)."""
    if "P" not in _CACHE:
        G = np.load(os.path.join(GOLDEN, "golden_generator.npz"))
        cfg = O.make_config(**{str(k): int(v) for k, v in zip(G["cfg_keys"], G["cfg_vals"])})
        _CACHE["P"] = (cfg, {k[3:]: torch.from_numpy(G[k]) for k in G.files if k.startswith("w::")})
    return _CACHE["P"]


def oracle_logits():
    """The oracle's fp32 logits of the golden set's 1360 rows, computed once."""
    if "z" not in _CACHE:
        cfg, P = golden_weights()
        rn, re_ = route_set()[:2]
        with torch.no_grad():
            _CACHE["z"] = O.ggnn_forward(P, cfg, torch.from_numpy(rn).float(), torch.from_numpy(re_).float())
    return _CACHE["z"]


def test_golden_is_what_its_docstring_says():
    G = golden()
    _, _, hot, row_mol = route_set()[:4]
    assert G["row_ll"].shape == G["row_ll_ref32"].shape == hot.shape == (1360,)
    assert G["mol_ll"].shape == (140,) and G["mol_kind"].shape == (140, 3)
    assert G["row_ll"].dtype == np.float64 and G["row_ll_ref32"].dtype == np.float32
    assert np.isfinite(G["row_ll"]).all() and np.isfinite(G["row_ll_ref32"]).all()
    assert -44.3 <= G["row_ll"].min() and G["row_ll"].max() <= -9e-7
    # the reference's linear-space fp32 expression agrees with fp64 log space where nothing underflows
    assert np.abs(G["row_ll_ref32"] - G["row_ll"]).max() <= 2e-7 * np.abs(G["row_ll"]).max()
    assert np.array_equal(G["w"], np.random.default_rng(int(G["w_seed"])).uniform(0.5, 1.5, 140).astype(np.float32))
    assert np.allclose(np.bincount(row_mol, weights=G["row_ll"]), G["mol_ll"], rtol=1e-12)


def test_restatement_on_the_oracles_logits_reproduces_the_golden():
    G = golden()
    _, _, hot, row_mol, _, _, dim_f_add, dim_f_conn = route_set()
    n_add, n_conn = LM.kind_dims(dim_f_add, dim_f_conn)
    assert n_add + n_conn + 1 == 625
    z = oracle_logits()
    slack = ORACLE_LOGITS_BAR * float(G["logit_absmax"])        # how far a logit may sit from the reference's
    assert float(z.abs().max()) <= float(G["logit_absmax"]) * (1 + ORACLE_LOGITS_BAR)
    h, rm = torch.from_numpy(hot), torch.from_numpy(row_mol)
    rows = LM.row_ll(z.double(), h)                              # fp64 on the fp32 logits: only `slack` is left
    err = (rows.numpy() - G["row_ll"])
    print(f"\nrows: max |err| {np.abs(err).max():.2e} (bound {2 * slack:.2e})")
    assert (np.abs(err) <= 2 * slack).all()                      # z[hot] and logsumexp(z) each move by <= slack
    n_rows = np.bincount(row_mol, minlength=140)
    mols = LM.molecule_ll(rows, rm, 140).numpy()
    assert (np.abs(mols - G["mol_ll"]) <= 2 * slack * n_rows).all()
    kinds = LM.molecule_kinds(rows, h, rm, 140, n_add, n_conn).numpy()
    assert (np.abs(kinds - G["mol_kind"]) <= 2 * slack * n_rows[:, None]).all()
    assert np.abs(kinds.sum(1) - mols).max() <= 1e-9
    # the terminate column is row 0 of every route, the only row whose hot index is the last one
    assert np.array_equal(LM.kind_of(h, n_add, n_conn).numpy() == 2, hot == 624)
    # fp32, as the device computes it: rounding of z - logsumexp(z) at the logits' magnitude on top
    rows32 = LM.row_ll(z, h).numpy()
    assert (np.abs(rows32 - G["row_ll"]) <= 2 * slack + 4 * 6e-8 * float(G["logit_absmax"])).all()


def test_restatement_gradients_reproduce_the_golden():
    G = golden()
    cfg, P = golden_weights()
    rn, re_, hot, row_mol = route_set()[:4]
    h, rm, w = torch.from_numpy(hot), torch.from_numpy(row_mol), torch.from_numpy(G["w"])
    z = oracle_logits().clone().requires_grad_(True)
    loss = LM.weighted_objective(z, h, rm, w)
    assert abs(float(loss.detach()) - float(G["loss"])) <= 1e-5 * abs(float(G["loss"]))
    (d_logits,) = torch.autograd.grad(loss, z)
    assert float(d_logits.sum(1).abs().max()) <= 1e-6            # every row: w_m (delta - softmax) / M sums to 0
    _, _, grads = O.forward_backward(P, cfg, torch.from_numpy(rn).float(), torch.from_numpy(re_).float(),
                                     torch.ones(rn.shape[0], 625), upstream=d_logits)
    for k, g in grads.items():
        ref = G["g::" + k].astype(np.float64)
        rel = float(np.abs(g.numpy() - ref).max() / max(np.abs(ref).max(), 1e-30))
        assert rel < 2e-5, (k, rel)                              # test_oracle_golden.py's bar on gradients


def test_sequential_sum_is_the_row_order_fp32_sum():
    rows = np.array([0.1, 0.2, 0.3, 1e8, -1e8, 0.5], np.float32)
    rm = np.array([0, 0, 0, 1, 1, -1])
    out = LM.sequential_sum(rows, rm, 3)
    assert out[0] == np.float32(np.float32(np.float32(0.1) + np.float32(0.2)) + np.float32(0.3))
    assert out[1] == 0 and out[2] == 0
    assert np.array_equal(LM.sequential_sum(rows[3:], rm[3:], 3, start=LM.sequential_sum(rows[:3], rm[:3], 3)), out)


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "graphinvent_amd.h")).read()
    assert re.search(r"#define GI_ABI_VERSION 18\b", header)
    for name in NEW_SYMBOLS:
        assert re.search(r"^int\s+%s\s*\(" % name, header, re.M), name
        assert name in L.SIGNATURES, name
    assert "gi_loglik.hip" in open(os.path.join(L.CSRC, "Makefile")).read()
    lib = L.load()                                               # binds every symbol of SIGNATURES or raises
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.gi_abi_version() == L.ABI_VERSION == 18
    assert (L.LL_ERR_HOT, L.LL_ERR_MOL, L.LL_ERR_ORDER) == tuple(
        int(re.search(r"#define GI_LL_ERR_%s (\d+)" % n, header).group(1)) for n in ("HOT", "MOL", "ORDER"))
    # host-side argument checks need no device
    assert lib.gi_row_loglik(None, 4, 1, 0, None, None, None, None, None) == -1       # W < 1
    assert lib.gi_row_loglik(None, 3, 1, 4, None, None, None, None, None) == -1       # pitch < W
    assert lib.gi_row_loglik(None, 4, 0, 4, None, None, None, None, None) == 0        # no rows: nothing to do
    assert lib.gi_mol_loglik_sum(None, None, None, 0, 5, 4, 2, 1, None, None, None, None) == 0
    assert lib.gi_route_rows_hot(None, 10, None) == -1


def test_public_functions_refuse_cpu_tensors():
    from graphinvent_amd import likelihood as LL
    _, _, hot, _, mn, me, dim_f_add, dim_f_conn = route_set()
    with pytest.raises(RuntimeError, match="CUDA"):
        LL.row_log_likelihood(torch.zeros(4, 625), torch.zeros(4, dtype=torch.int32))
    nodes, edges = torch.from_numpy(mn[:3]), torch.from_numpy(me[:3])
    model = lambda n, e: torch.zeros(n.shape[0], 625)           # never reached
    with pytest.raises(RuntimeError, match="CUDA"):
        LL.molecule_log_likelihood(model, nodes, edges, dim_f_add, dim_f_conn)
    with pytest.raises(RuntimeError, match="CUDA"):
        LL.weighted_log_likelihood_backward(model, nodes, edges, dim_f_add, dim_f_conn, torch.ones(3))
    with pytest.raises(ValueError, match="invalid must be"):
        LL.molecule_log_likelihood(model, nodes, edges, dim_f_add, dim_f_conn, invalid="ignore")
