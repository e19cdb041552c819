"""-m gpu: the MNN model across dimensions, depths and pass counts, and its kernels at their edges.

tests/test_mnn_gpu.py runs MNN at two shapes (the tiny golden; GDB-13 defaults, H = M = 100, Fe = 3, 3 passes, depth 4).
Its message steps in the shared driver (csrc/gi_model.hip msg_fwd_mnn / msg_bwd_mnn / msg_wgrad_mnn) and its kernels (csrc/gi_mnn.hip, templated on Fe = 1 .. 8)
branch on more than that:

  fe1 / fe4 / fe8   every bond-type count the templates are built for, with EVERY type present (synthetic.make_batch
                    gives the types beyond the third probability 0: the bonds are redrawn uniformly)
  h_ne_m            H = 256, M = 64: H Fe = 768 columns of typed sums, the dS GEMM with N = 768
  n88               ChEMBL-shaped graphs, B = 64
  passes1           the `p > 0` block (dS GEMM + transposed typed sum) never runs
  passes16          the driver's pass limit; ill-conditioned in fp32, see its test
  depth0 / depth11  GlobalReadout's stacks one Linear each / at the depth limit
  passes0           no message GEMM, no GRU: their gradients stay None (module path)
  no_edges          3 passes over isolated atoms and empty graphs: E = 0
  gen_slot0         the generation loop's dummy graph (all-ones node row, self-loop, every bond type on one pair) and
                    an ordinary pair with two bond types, in a training step
  b1                B = 1, and row independence

Protocol = tests/test_mnn_gpu.py::test_b1000_matches_pinned_oracle in the loop of tests/test_dims_gpu.py: logits, loss
and every gradient tensor at 1e-4 (max |d| / max |ref| per tensor) against the fp32 oracle's autograd with the SELU
branches pinned to the HIP forward's (ties only), every row also against the plain oracle (MNN has no gather, so no
masked-graph energy quanta), in the three arithmetic modes, with the pipes `gi_prof_pipes` reports.

The kernels only add, in a documented fixed order, so they are compared BIT FOR BIT with fp32 numpy mirrors that add in
the same order (tests/mnn_oracle.py; tests/test_mnn_cpu.py holds the mirrors within (terms - 1) 2^-24 sum |terms| of
the fp64 sums), and within that same bound of the fp64 sums themselves."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from graphinvent_amd import lib as L, synthetic
from graphinvent_amd.gnn import mpnn
from oracle import ggnn_oracle as O
from tests import mnn_oracle as MO
from tests.pins import TIE_TOL, OraclePins, graph_arrays
from tests.ref_dataflow import compact
from tests.test_depths_gpu import check_pipes, has_wide_layer
from tests.test_dims_gpu import MODES, _pipes, _set_mode
from tests.test_mnn_gpu import mnn_signs
from tests.test_model_gpu import to_dev

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4
GDB13 = synthetic.SHAPES["gdb13"]
CHEMBL = synthetic.SHAPES["chembl"]
EINVAL = -1


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def mnn_wide(cfg) -> bool:
    """tests/test_depths_gpu.has_wide_layer for a config without gather stacks."""
    return has_wide_layer(dict(cfg, gather_att_depth=0, gather_att_hidden_dim=0, gather_emb_depth=0,
                               gather_emb_hidden_dim=0))


def build_mnn(cfg, P):
    m = mpnn.MNN(MO.as_constants(dict(cfg, device="cuda")))
    m.load_state_dict(P)
    return m.to(DEV).train()


def hip_step(lib, cfg, P, n8, e8, a8):
    """One raw MNN training forward + backward under the profiler.  Returns (logits, loss, grads by key, SELU signs,
    compact-graph arrays, launches per pipe)."""
    m = build_mnn(cfg, P)
    params = list(m.parameters())
    nodes, edges, tgt = to_dev(n8, e8, a8)
    torch.cuda.synchronize()
    lib.gi_prof_enable(1)
    try:
        out, tape = mpnn.ggnn_forward_raw(m.constants, nodes, edges, params, L.KIND_MNN)
        # (read back BEFORE the backward, which forms the last layers' dZ in place over their outputs)
        signs = mnn_signs(tape[0], tape[1], tape[2], out)
        g = graph_arrays(tape[1])
        o_leaf = out.detach().clone().requires_grad_(True)
        loss = O.kl_loss(o_leaf, tgt)
        loss.backward()
        grads, _ = mpnn.ggnn_backward_raw(tape, out, o_leaf.grad, params)
        torch.cuda.synchronize()
        ms = (C.c_double * 2)(); busy = (C.c_double * 2)(); work = (C.c_double * 2)(); nl = (C.c_int * 2)()
        L.check(lib.gi_prof_collect(ms, busy, work, nl), "gi_prof_collect")
        pipes = _pipes(lib)
    finally:
        lib.gi_prof_enable(0)
    names = [k for k, _ in m.named_parameters()]
    assert names == list(MO.param_shapes(cfg))
    return out.detach().cpu(), float(loss.detach()), dict(zip(names, (x.detach().cpu() for x in grads))), signs, g, pipes


def oracle_pinned(cfg, P, n8, e8, a8, signs, g):
    """The fp32 MNN oracle's forward + autograd with the SELU branches of `signs`; the pin may only resolve ties."""
    pin = OraclePins(signs, g, n8, e8, "MNN")
    O.SELU_BRANCH_HOOK = pin
    try:
        ref = MO.forward_backward(P, cfg, *(torch.from_numpy(x).float() for x in (n8, e8, a8)))
    finally:
        O.SELU_BRANCH_HOOK = None
    assert pin.max_flipped_abs < TIE_TOL and pin.flipped <= 1e-6 * pin.total, (pin.flipped, pin.total)
    return ref


def assert_mnn_parity(name, mode, cfg, P, n8, e8, a8, out, loss, grads, signs, g):
    o_ref, l_ref, g_ref = oracle_pinned(cfg, P, n8, e8, a8, signs, g)
    worst = [(rel(out, o_ref), "logits"), (abs(loss - float(l_ref)) / abs(float(l_ref)), "loss")]
    for k, gr in grads.items():
        if g_ref[k] is None:                                   # 0 passes: never read by the forward
            assert not bool(gr.any()), (name, mode, k)
        else:
            worst.append((rel(gr, g_ref[k]), k))
    print(f"[{name}/{mode}] worst vs the pinned fp32 oracle: {max(worst)}")
    assert max(worst)[0] < TOL, (name, mode, sorted(worst)[-3:])
    with torch.no_grad():
        plain = MO.mnn_forward(P, cfg, *(torch.from_numpy(x).float() for x in (n8, e8)))
    assert rel(out, plain) < TOL, (name, mode)
    return o_ref, l_ref, g_ref


def run_mnn_parity(name, cfg, n8, e8, a8, seed=31, wide=None):
    """The three-mode loop of tests/test_dims_gpu.py for an MNN case.  Returns the fp32 mode's (grads, pipes report)."""
    P = MO.init_params(cfg, seed=seed)
    wide = mnn_wide(cfg) if wide is None else wide
    lib = L.load()
    was = lib.gi_bf3_enable(-1), lib.gi_x2_enable(-1)
    old_threads = torch.get_num_threads()
    torch.set_num_threads(max(1, min(32, torch.get_num_threads())))
    report, grads = {}, None
    try:
        for mode in MODES:
            _set_mode(lib, mode)
            out, loss, grads, signs, g, report[mode] = hip_step(lib, cfg, P, n8, e8, a8)
            check_pipes(name, mode, report[mode], wide)
            assert_mnn_parity(name, mode, cfg, P, n8, e8, a8, out, loss, grads, signs, g)
    finally:
        lib.gi_prof_enable(0)
        lib.gi_bf3_enable(was[0]); lib.gi_x2_enable(was[1])
        torch.set_num_threads(old_threads)
    print(f"\n[{name}] GEMM-family launches per matrix pipe and mode: {report}")
    return P, grads


# ---- the model ------------------------------------------------------------------------------------------------------
#: every readout stack at the depth limit, narrow widths, mlp1 wide enough for the 16-bit pipes (test_depths_gpu.DEEP)
DEEP = dict(mlp1_depth=L.MODEL_MAX_DEPTH, mlp2_depth=L.MODEL_MAX_DEPTH, hidden_node_features=32, message_size=32,
            mlp1_hidden_dim=256, mlp2_hidden_dim=64)
#: name -> (shape, B, bond types, overrides of the shape's default MNN config)
CASES = {
    "fe1": (GDB13, 420, 1, {}),
    "fe4": (GDB13, 420, 4, {}),
    "fe8": (GDB13, 420, L.GI_MAX_GROUPS, {}),
    "h_ne_m": (GDB13, 420, 3, dict(hidden_node_features=256, message_size=64)),
    "n88": (CHEMBL, 64, 3, {}),
    "passes1": (GDB13, 420, 3, dict(message_passes=1)),
    "depth0": (GDB13, 420, 3, dict(mlp1_depth=0, mlp2_depth=0)),
    "depth11": (GDB13, 420, 3, DEEP),
}


def case(name, seed=51):
    shape, B, Fe, over = {**CASES, "passes16": (GDB13, 420, 3, dict(message_passes=L.MODEL_MAX_PASSES)),
                          "passes0": (GDB13, 64, 3, dict(message_passes=0)),
                          "plain": (GDB13, 420, 3, {})}[name]
    sh = dict(shape, n_edge_features=Fe)
    cfg = MO.mnn_config(sh["n_atom_types"], sh["n_formal_charge"], sh["max_n_nodes"], Fe, **over)
    n8, e8, a8 = synthetic.make_batch(B, **sh, seed=seed)
    assert a8.shape[1] == O.apd_width(cfg)                     # (the APD width follows the config's bond-type count)
    if name.startswith("fe"):
        e8 = MO.redraw_bond_types(e8, np.random.default_rng(seed + 1))
        assert e8.any((0, 1, 2)).all()                         # every bond type occurs
    return cfg, (n8, e8, a8)


@pytest.mark.parametrize("name", list(CASES))
def test_mnn_parity_across_dimensions_depths_and_passes(name):
    cfg, (n8, e8, a8) = case(name)
    assert n8.shape[0] * n8.shape[1] >= 2560
    run_mnn_parity(name, cfg, n8, e8, a8)


@functools.lru_cache(maxsize=None)
def _passes16():
    """The case and both plain oracles (fp32 and fp64), computed once for the three modes."""
    cfg, (n8, e8, a8) = case("passes16")
    P = MO.init_params(cfg, seed=31)
    t = lambda x, dt: torch.from_numpy(x).to(dt)
    old_threads = torch.get_num_threads()
    torch.set_num_threads(max(1, min(32, torch.get_num_threads())))
    try:
        ref32 = MO.forward_backward(P, cfg, *(t(x, torch.float32) for x in (n8, e8, a8)))
        ref64 = MO.forward_backward({k: v.double() for k, v in P.items()}, cfg,
                                    *(t(x, torch.float64) for x in (n8, e8, a8)))
    finally:
        torch.set_num_threads(old_threads)
    return cfg, (n8, e8, a8), P, ref32, ref64


@pytest.mark.parametrize("mode", MODES)
def test_sixteen_passes_within_the_fp32_conditioning(mode):
    """16 passes (the driver's limit).  Sixteen GRU updates can make single gradient tensors ill-conditioned in fp32 (a
    SELU branch that flips between two correct fp32 evaluations moves a tensor by up to ~1e-2), so the case carries
    the fall-back of tests/test_depths_gpu.py::test_deepest_model_within_the_fp32_conditioning.  Measured on the CPU
    for this batch (B = 420, batch seed 51, weights seed 31), UNPINNED fp32 MNN oracle against the fp64 oracle: logits
    1.3e-6, loss 5.6e-7 absolute (of 6.03), the gradients as one vector 6.9e-7, worst single tensor 2.2e-6
    (APDReadout.fConnNet1.seq.9.weight); batch seed 3: 1.2e-6 / 5.3e-7 / 8.0e-7 / 3.4e-6 (docs/MEASUREMENTS_LOG.md).
    First the pinned 1e-4 protocol; where the PINNED fp32 oracle is itself further than 2.5e-5 from fp64 (logits or
    any gradient tensor), the mode is held against the fp64 oracle instead: logits, loss and the gradients as one
    vector within 4x the unpinned fp32 oracle's own error (at least 1e-4), every single tensor below 0.75.  Which
    protocol applies is decided by the oracles alone, never by the HIP result; both sets of figures are printed.
    Measured on the MI355X: the pinned fp32 oracle is 3.2e-4 from fp64 in APDReadout.fConnNet1.seq.6.weight with the
    fp16x2 and the fp32-MFMA forward's branches (one SELU tie that fp64 resolves the other way) and 2.3e-6 with the
    bf16x3 forward's, so two modes take the fp64 protocol and one the pinned one; the HIP gradients are within 3.3e-6 of
    the pinned oracle and 2.4e-6 (as one vector) of fp64 in all three."""
    name = "passes16"
    cfg, (n8, e8, a8), P, (o32, l32, g32), (o64, l64, g64) = _passes16()
    names = list(P)
    ref64 = torch.cat([g64[k].flatten() for k in names])
    l2 = lambda gs: float((torch.cat([gs[k].double().flatten() for k in names]) - ref64).norm() / ref64.norm())
    own = dict(logits=rel(o32, o64), loss=abs(float(l32) - float(l64)), vector=l2(g32),
               tensor=max((rel(g32[k], g64[k]), k) for k in names))
    print(f"\n[{name}] unpinned fp32 oracle vs fp64 oracle: {own}")
    old_threads = torch.get_num_threads()
    torch.set_num_threads(max(1, min(32, torch.get_num_threads())))
    lib = L.load()
    was = lib.gi_bf3_enable(-1), lib.gi_x2_enable(-1)
    try:
        _set_mode(lib, mode)
        out, loss, grads, signs, g, pipes = hip_step(lib, cfg, P, n8, e8, a8)
        check_pipes(name, mode, pipes, mnn_wide(cfg))
        op, lp, gp = oracle_pinned(cfg, P, n8, e8, a8, signs, g)
    finally:
        lib.gi_prof_enable(0)
        lib.gi_bf3_enable(was[0]); lib.gi_x2_enable(was[1])
        torch.set_num_threads(old_threads)
    pinned = max([(rel(op, o64), "logits")] + [(rel(gp[k], g64[k]), k) for k in names])
    hip = max([(rel(out, op), "logits")] + [(rel(grads[k], gp[k]), k) for k in names])
    print(f"[{name}/{mode}] pinned fp32 oracle vs fp64: {pinned}; HIP vs pinned: {hip}; "
          f"HIP vs fp64: logits {rel(out, o64):.2e}, gradient vector {l2(grads):.2e}")
    if pinned[0] <= 2.5e-5:
        assert hip[0] < TOL and abs(loss - float(lp)) < TOL * abs(float(lp)), (mode, hip)
        return
    assert rel(out, o64) < 4 * max(own["logits"], 2.5e-5), (mode, rel(out, o64), own)
    assert abs(loss - float(l64)) < 4 * max(own["loss"], 2.5e-5 * float(l64)), (mode, loss, float(l64), own)
    assert l2(grads) < 4 * max(own["vector"], 2.5e-5), (mode, l2(grads), own)
    for k in names:
        assert rel(grads[k], g64[k]) < 0.75, (mode, k, rel(grads[k], g64[k]), rel(g32[k], g64[k]))


UNUSED_AT_0_PASSES = {"message_weights", "gru.weight_ih", "gru.weight_hh", "gru.bias_ih", "gru.bias_hh"}


def test_zero_passes_leave_the_message_parameters_without_gradient():
    """tests/test_depths_gpu.py's protocol for MNN: at 0 passes message_weights and gru.* keep .grad None on both
    autograd paths (msg_wgrad_mnn's memset of dW must not surface), a held gradient is untouched, torch.optim.Adam
    leaves them where they are, every other gradient is within 1e-4 of the oracle's."""
    cfg, (n8, e8, a8) = case("passes0")
    P = MO.init_params(cfg, seed=32)
    _, _, g32 = MO.forward_backward(P, cfg, *(torch.from_numpy(x).float() for x in (n8, e8, a8)))
    unused = {k for k, v in g32.items() if v is None}
    assert unused == UNUSED_AT_0_PASSES
    nodes, edges, tgt = to_dev(n8, e8, a8)
    for autograd_params in (False, True):
        m = build_mnn(cfg, P)
        m.autograd_params = autograd_params
        O.kl_loss(m(nodes, edges), tgt).backward()
        for k, p in m.named_parameters():
            if k in unused:
                assert p.grad is None, (autograd_params, k)
            else:
                assert p.grad is not None and float((p.grad.cpu() - g32[k]).abs().max()) <= \
                    1e-4 * max(float(g32[k].abs().max()), 1e-30), (autograd_params, k)
        held = {k: torch.full_like(p, 7.0) for k, p in m.named_parameters() if k in unused}
        for k, p in m.named_parameters():
            if k in unused:
                p.grad = held[k].clone()
        O.kl_loss(m(nodes, edges), tgt).backward()
        for k, p in m.named_parameters():
            if k in unused:
                assert torch.equal(p.grad, held[k]), (autograd_params, k)
    m = build_mnn(cfg, P)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-4)
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    O.kl_loss(m(nodes, edges), tgt).backward()
    opt.step()
    for k, p in m.named_parameters():
        assert torch.equal(p.detach(), before[k]) == (k in unused), k


def test_three_passes_over_a_batch_without_any_edge():
    """Isolated atoms and empty graphs only (E = 0): the typed sums are all 0, the GRU updates nothing, the dS GEMM and
    the transposed typed sum are skipped.  Logits and every gradient match the oracle; the gradients of
    message_weights and gru.* are tensors of exact zeros, not None (the forward does read them)."""
    cfg, (n8, e8, a8) = case("plain", seed=52)
    e8 = np.zeros_like(e8)
    P, grads = run_mnn_parity("no_edges", cfg, n8, e8, a8)
    for k in UNUSED_AT_0_PASSES:
        assert grads[k].shape == P[k].shape and not bool(grads[k].any()), k
    m = build_mnn(cfg, P)
    nodes, edges, tgt = to_dev(n8, e8, a8)
    O.kl_loss(m(nodes, edges), tgt).backward()
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        if k in UNUSED_AT_0_PASSES:
            assert not bool(p.grad.any()), k


def test_training_step_on_the_generation_dummy_graph_and_a_two_type_pair():
    """Graph 0 is the generation loop's dummy (GraphGenerator.py:133: all-ones node row, a self-loop, every bond type
    set on that pair = Fe parallel self-edges); another graph has an ordinary pair carrying two bond types.  The
    oracle's einsum sums the types of a pair, the HIP path counts one edge per set entry."""
    cfg, (n8, e8, a8) = case("plain", seed=53)
    n8[0] = 0; e8[0] = 0
    n8[0, 0, :] = 1
    e8[0, 0, 0, :] = 1
    b = 1 + int(np.nonzero(n8[1:, 1].any(1))[0][0])            # the first other graph with at least two atoms
    e8[b, 0, 1, :] = 0; e8[b, 1, 0, :] = 0
    e8[b, 0, 1, [0, 2]] = 1; e8[b, 1, 0, [0, 2]] = 1
    g = compact(n8, e8)
    assert g["err"] & 8 and g["E"] > int(e8.any(3).sum())      # parallel edges: more edges than bonded pairs
    run_mnn_parity("gen_slot0", cfg, n8, e8, a8)


def test_batch_of_one_and_row_independence():
    """B = 1 in a training step against the oracle; then (tests/test_model_gpu.py's criterion) every graph of a
    B = 1200 batch gets the logits it gets in a batch of its own third, to 1e-5: only summation orders may differ."""
    cfg, (n8, e8, a8) = case("plain", seed=54)
    b = int(np.nonzero(e8.reshape(e8.shape[0], -1).any(1))[0][0])
    P, _ = run_mnn_parity("b1", cfg, n8[b:b + 1], e8[b:b + 1], a8[b:b + 1], wide=False)
    m = build_mnn(cfg, P)
    n8, e8, a8 = synthetic.make_batch(1200, **GDB13, seed=55)
    nodes, edges, tgt = to_dev(n8, e8, a8)
    out = m(nodes, edges)
    O.kl_loss(out, tgt).backward()
    assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    with torch.no_grad():
        part = m(nodes[400:800].contiguous(), edges[400:800].contiguous())
    assert rel(out.detach()[400:800], part) < 1e-5


# ---- kernels --------------------------------------------------------------------------------------------------------
SENTINEL = 7.0


def _i32(x):
    x = np.ascontiguousarray(np.asarray(x, dtype=np.int32))
    return torch.from_numpy(x).to(DEV) if x.size else torch.zeros(1, dtype=torch.int32, device=DEV)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


INT_KEYS = ("u_src", "in_perm", "seg_off", "type_off", "out_perm", "src_off", "mu_off", "mu_dst", "cidx", "slot_of")


def _typed_sum(lib, hd, ldh, ints, R, H, Fe, out, ldo):
    return lib.gi_typed_seg_sum(hd.data_ptr(), ldh, ints["u_src"].data_ptr(), ints["in_perm"].data_ptr(),
                                ints["seg_off"].data_ptr(), ints["type_off"].data_ptr(), R, H, Fe, out.data_ptr(), ldo,
                                _stream())


def _typed_sum_t(lib, dSd, lds, ints, R, H, Fe, dh, lddh, accumulate):
    return lib.gi_typed_seg_sum_t(dSd.data_ptr(), lds, ints["out_perm"].data_ptr(), ints["src_off"].data_ptr(),
                                  ints["mu_off"].data_ptr(), ints["mu_dst"].data_ptr(), ints["type_off"].data_ptr(), R,
                                  H, Fe, dh.data_ptr(), lddh, accumulate, _stream())


@pytest.mark.parametrize("name,H", [(name, H) for name, hs in MO.KERNEL_CASES.items() for H in hs])
def test_typed_sums_bit_for_bit_with_their_mirrors(name, H):
    lib = L.load()
    n, e, nodedup = MO.kernel_case(name)
    Fe = e.shape[3]
    g = compact(n, e, nodedup=nodedup)
    R = g["S"] + 1
    if name.startswith("fe"):
        assert (np.diff(g["type_off"]) > 0).all()              # every template branch of row_type is taken
    if name.startswith("hub"):
        assert np.diff(g["seg_off"]).max() == 127
        assert (name == "hub_alone" and R == 129) or R * ((H + 3) // 4) > 3 * 256
    ldh, lds = ((H + 3) & ~3) + 4, ((H * Fe + 3) & ~3) + 4     # pitches with spare columns
    rng = np.random.default_rng(H)
    h = rng.standard_normal((R, ldh)).astype(np.float32)
    h[R - 1] = 0.0
    ints = {k: _i32(g[k]) for k in INT_KEYS}
    out = torch.full((R, lds), SENTINEL, device=DEV)
    L.check(_typed_sum(lib, _dev(h), ldh, ints, R, H, Fe, out, lds), "gi_typed_seg_sum")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    hH = np.ascontiguousarray(h[:, :H])
    assert np.array_equal(got[:, :H * Fe], MO.typed_sums_mirror(hH, g, Fe))
    ref = MO.typed_sums(hH.astype(np.float64), g["in_perm"], g["u_src"], MO.u_types(g), g["seg_off"], Fe)
    assert (np.abs(got[:, :H * Fe] - ref) <= MO.typed_sums_bound(hH, g, Fe)).all()
    assert (got[:, H * Fe:] == SENTINEL).all()                 # nothing written past H * Fe
    assert not got[np.diff(g["seg_off"]) == 0, :H * Fe].any()  # rows without in-edges, row S among them: exactly 0
    # the transpose, overwriting and accumulating
    dS = rng.standard_normal((R, lds)).astype(np.float32)
    dh0 = rng.standard_normal((R, ldh)).astype(np.float32)
    dSH = np.ascontiguousarray(dS[:, :H * Fe])
    ref_t, terms, mag = MO.typed_sums_t(dSH.astype(np.float64), g, Fe)
    for accumulate in (0, 1):
        dh = _dev(dh0)
        L.check(_typed_sum_t(lib, _dev(dS), lds, ints, R, H, Fe, dh, ldh, accumulate), "gi_typed_seg_sum_t")
        torch.cuda.synchronize()
        got_t = dh.cpu().numpy()
        assert np.array_equal(got_t[:, H:], dh0[:, H:]), accumulate          # columns >= H are never touched
        want = MO.typed_sums_t_mirror(dSH, g, Fe, np.ascontiguousarray(dh0[:, :H]) if accumulate else None)
        assert np.array_equal(got_t[:, :H], want), accumulate
        if accumulate:
            assert (np.abs(got_t[:, :H] - (ref_t + dh0[:, :H])) <=
                    (terms * 2.0 ** -24)[:, None] * (mag + np.abs(dh0[:, :H]))).all()
        else:
            assert (np.abs(got_t[:, :H] - ref_t) <= (np.maximum(terms - 1, 0) * 2.0 ** -24)[:, None] * mag).all()


@pytest.mark.parametrize("N", [1, 13, 88, 128])
@pytest.mark.parametrize("H", [1, 10, 50])
def test_graph_sum_fwd_bit_for_bit_every_destination_subset(N, H):
    lib = L.load()
    B = 7
    assert (B * H) % 256
    n, e, _ = synthetic.make_batch(B, N, 3, 2, 3, seed=N, frac_empty=0.15, frac_single=0.15)
    g = compact(n, e)
    R = g["S"] + 1
    ld = ((H + 3) & ~3) + 4
    h = np.random.default_rng(N + H).standard_normal((R, ld)).astype(np.float32)
    h[R - 1] = 0.0
    hH = np.ascontiguousarray(h[:, :H])
    want = MO.graph_sum_mirror(hH, g["cidx"], B, N)
    c = g["cidx"].reshape(B, N)
    ref, mag = hH.astype(np.float64)[c].sum(1), np.abs(hH.astype(np.float64))[c].sum(1)
    hd, cidx = _dev(h), _i32(g["cidx"])
    lds, offs = (H + 9, H + 2, H), (3, 1, 0)                   # offset destinations, odd pitches
    for nulls in ((), (0,), (1,), (2,), (0, 1, 2)):
        outs = [torch.full((B, lds[i]), SENTINEL, device=DEV) for i in range(3)]
        ptrs = [0 if i in nulls else outs[i].data_ptr() + 4 * offs[i] for i in range(3)]
        L.check(lib.gi_graph_sum_fwd(hd.data_ptr(), ld, cidx.data_ptr(), B, N, H, ptrs[0], lds[0], ptrs[1], lds[1],
                                     ptrs[2], lds[2], _stream()), "gi_graph_sum_fwd")
        torch.cuda.synchronize()
        for i in range(3):
            got = outs[i].cpu().numpy()
            if i in nulls:
                assert (got == SENTINEL).all(), (nulls, i)
                continue
            assert np.array_equal(got[:, offs[i]:offs[i] + H], want), (nulls, i)
            assert (np.abs(got[:, offs[i]:offs[i] + H] - ref) <= (N - 1) * 2.0 ** -24 * mag).all()
            assert (got[:, :offs[i]] == SENTINEL).all() and (got[:, offs[i] + H:] == SENTINEL).all(), (nulls, i)


@pytest.mark.parametrize("case_name", ["graphs", "nodedup", "empty"])
@pytest.mark.parametrize("H", [1, 10, 50])
def test_graph_sum_bwd_every_source_subset_and_accumulation(case_name, H):
    """dh[c] (+)= dg0[b] + dg1[b] + dg2[b] in that order onto 0 (fp32, so exact against numpy); row S is zeroed when
    not accumulating and untouched when accumulating; all three sources NULL give zeros / leave dh unchanged."""
    lib = L.load()
    n, e, nodedup = MO.kernel_case("graphs" if case_name == "empty" else case_name)
    if case_name == "empty":                                   # S = 0: only the zero row
        n[:] = 0; e[:] = 0
    B, N = n.shape[:2]
    g = compact(n, e, nodedup=nodedup)
    S = g["S"]
    assert (S == 0) == (case_name == "empty")
    R, ld, ldg = S + 1, ((H + 3) & ~3) + 4, H + 3
    rng = np.random.default_rng(H)
    dg = [rng.standard_normal((B, ldg)).astype(np.float32) for _ in range(3)]
    dh0 = rng.standard_normal((R, ld)).astype(np.float32)
    dgd, slot_of = [_dev(x) for x in dg], _i32(g["slot_of"])
    graph_of = g["slot_of"].astype(np.int64) // N
    for accumulate in (0, 1):
        for nulls in ((), (0,), (1,), (2,), (0, 1, 2)):
            dh = _dev(dh0)
            ptrs = [0 if i in nulls else dgd[i].data_ptr() for i in range(3)]
            L.check(lib.gi_graph_sum_bwd(ptrs[0], ldg, ptrs[1], ldg, ptrs[2], ldg, slot_of.data_ptr(), S, N, H,
                                         dh.data_ptr(), ld, accumulate, _stream()), "gi_graph_sum_bwd")
            torch.cuda.synchronize()
            got = dh.cpu().numpy()
            v = np.zeros((B, H), np.float32)
            for i in range(3):
                if i not in nulls:
                    v = v + dg[i][:, :H]
            want = dh0.copy()
            want[:S, :H] = (dh0[:S, :H] + v[graph_of]) if accumulate else v[graph_of]
            if not accumulate:
                want[S, :H] = 0.0
            assert np.array_equal(got, want), (accumulate, nulls)


def test_kernel_refusals_leave_the_output_untouched():
    """Bad arguments return GI_EINVAL before anything is launched; rows = 0 returns 0 and writes nothing."""
    lib = L.load()
    n, e, _ = MO.kernel_case("graphs")
    g = compact(n, e)
    Fe, H, R = 3, 13, g["S"] + 1
    ldh, lds = 16, 40
    ints = {k: _i32(g[k]) for k in INT_KEYS}
    hd = torch.randn(R, ldh + 4, device=DEV)
    dSd = torch.randn(R, lds + 4, device=DEV)
    out = torch.full((R + 1, lds + 4), SENTINEL, device=DEV)
    untouched = lambda: bool((out == SENTINEL).all())
    bad_fwd = dict(ldh_odd=dict(ldh=ldh + 1), ldo_odd=dict(ldo=lds + 1), ldo_short=dict(ldo=H * Fe - 3),
                   fe0=dict(Fe=0), fe9=dict(Fe=L.GI_MAX_GROUPS + 1), out_misaligned=dict(shift=4))
    for tag, kw in bad_fwd.items():
        a = dict(dict(ldh=ldh, ldo=lds, Fe=Fe, shift=0), **kw)
        view = out.view(-1)[a["shift"] // 4:]
        assert _typed_sum(lib, hd, a["ldh"], ints, R, H, a["Fe"], view, a["ldo"]) == EINVAL, tag
        torch.cuda.synchronize()
        assert untouched(), tag
    bad_t = dict(lds_short=dict(lds=H * Fe - 1), lddh_short=dict(lddh=H - 1), fe0=dict(Fe=0),
                 fe9=dict(Fe=L.GI_MAX_GROUPS + 1))
    for tag, kw in bad_t.items():
        a = dict(dict(lds=lds, lddh=ldh, Fe=Fe), **kw)
        for accumulate in (0, 1):
            assert _typed_sum_t(lib, dSd, a["lds"], ints, R, H, a["Fe"], out, a["lddh"], accumulate) == EINVAL, tag
        torch.cuda.synchronize()
        assert untouched(), tag
    assert _typed_sum(lib, hd, ldh, ints, 0, H, Fe, out, lds) == 0
    assert _typed_sum_t(lib, dSd, lds, ints, 0, H, Fe, out, ldh, 0) == 0
    torch.cuda.synchronize()
    assert untouched()
