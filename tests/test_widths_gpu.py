"""-m gpu: model-level parity at hidden and message widths that are NOT multiples of 4.

Every other model test uses H / M in {16/12, 24/20, 24/24, 32/32, 100/100, 128/128, 256/256}.  The reference accepts
any width, and the driver (csrc/gi_model.hip) branches on `width & 3`:

  GRU forward    gi_gru_fused_ok needs H % 4 == 0 and M % 4 == 0; otherwise both projections go into one GEMM launch and
                 the scalar gru_gates_fwd_kernel follows ("widths that are not multiples of 4")
  GRU backward   the vector gate kernel and the folded d h scatter (fuse_scatter) need H % 4 == 0; otherwise the scalar
                 gate backward and separate gi_seg_sum launches run
  row pitches    every pitch is rounded up to 4 floats; seg_sum, seg_softmax and typed_seg_sum move whole 16-byte groups,
                 so the pad columns take part, and the padded rows reach GEMMs with odd K and ld (MNN's message weight is
                 used as stored: ldb = H Fe), the chain kernels, the 16-bit-pipe layers with odd fan-in / fan-out, the
                 gather readout (gather_width % 4 != 0), the slot glue and the flat gradient bucket (segments padded to 4)

Kernel tests touch single pieces (test_gru_gates_* at H = 18, GEMMs at K = 685, typed_seg_sum at H = 13); the hand-over
between kernels at such widths is what these cases check.  Residues 1, 2 and 3 of both H and M occur.

Protocol = tests/test_dims_gpu.py (GGNN, AttentionGGNN) and tests/test_mnn_dims_gpu.py (MNN): logits, loss and every
gradient tensor at 1e-4 against the fp32 oracle's autograd with SELU branches and masked-graph energy quanta pinned to
the HIP forward's (ties only), live rows also against the plain oracle, three arithmetic modes, pipes asserted;
GDB-13-shaped batches of 420 graphs (>= 2 560 node rows).

Found by these cases: with an odd gather_width (ggnn_r2_r1, ggnn_r3_r2, att_r2_r1) the driver summed the zero row's
per-graph partial sums of the gather backward with a pitch rounded up to 4 floats, while gi_gather_readout_bwd writes
them dense ([B, 2 G]): every gather.att_nn / gather.emb_nn gradient except the first layers' weights was wrong.

Widths below 4: the HIP path needs every Linear's fan-in and fan-out, the message size and the hidden size to fill one
16-byte vector (gi_gemm takes rows narrower than that only where they are stored padded, and weights are used as
PyTorch stores them; chain_fits and the fused GRU need >= 4 too).  EVERY such key is refused at construction with a
ValueError naming it (gnn/mpnn.py _check_limits, tests/test_limits_cpu.py) instead of failing inside a
forward; the smallest accepted widths (4 everywhere) are held to the parity protocol here."""
import ctypes as C

import numpy as np
import pytest
import torch

from graphinvent_amd import lib as L, synthetic
from graphinvent_amd.gnn import mpnn
from oracle import ggnn_oracle as O
from tests import mnn_oracle as MO
from tests import pins
from tests.test_depths_gpu import build, check_pipes, has_wide_layer
from tests.test_dims_gpu import MODES, _pipes, _set_mode
from tests.test_mnn_dims_gpu import build_mnn, run_mnn_parity
from tests.test_model_gpu import assert_parity_with_both_pins, fully_masked_rows, to_dev

pytestmark = pytest.mark.gpu
DEV = "cuda"
GDB13 = synthetic.SHAPES["gdb13"]

R2_R1 = dict(hidden_node_features=50, message_size=37, gather_width=99, gather_att_hidden_dim=201,
             gather_emb_hidden_dim=203, mlp1_hidden_dim=251, mlp2_hidden_dim=101)
#: name -> (model, overrides of the GDB-13 default config); every H >= Fn = 8
CASES = {
    "ggnn_r2_r1": ("GGNN", dict(R2_R1, enn_hidden_dim=45)),
    "ggnn_r3_r2": ("GGNN", dict(hidden_node_features=27, message_size=26, enn_hidden_dim=30, gather_width=33,
                                gather_att_hidden_dim=65, gather_emb_hidden_dim=65, mlp1_hidden_dim=65,
                                mlp2_hidden_dim=65)),                     # (no wide layer)
    "ggnn_h4_m_odd": ("GGNN", dict(hidden_node_features=48, message_size=35)),   # only M breaks the fused GRU
    "att_r2_r1": ("AttGGNN", dict(R2_R1, msg_hidden_dim=45, att_hidden_dim=43)),
    # H Fe = 150: ldS = 152, and the rows of the stored message weight (ldb = 150) are not 16-byte aligned
    "mnn_r2_r1": ("MNN", dict(hidden_node_features=50, message_size=37, mlp1_hidden_dim=251, mlp2_hidden_dim=101)),
    "mnn_r1": ("MNN", dict(hidden_node_features=33, message_size=50)),
}
#: the smallest widths the HIP models accept (below: refused at construction)
MIN4 = {"GGNN": dict(message_size=4, gather_width=4, enn_hidden_dim=4, gather_att_hidden_dim=4, gather_emb_hidden_dim=4,
                     mlp1_hidden_dim=4, mlp2_hidden_dim=4),
        "AttGGNN": dict(message_size=4, gather_width=4, msg_hidden_dim=4, att_hidden_dim=4, gather_att_hidden_dim=4,
                        gather_emb_hidden_dim=4, mlp1_hidden_dim=4, mlp2_hidden_dim=4),
        "MNN": dict(message_size=4, mlp1_hidden_dim=4, mlp2_hidden_dim=4)}
#: the issue's sub-vector widths
BELOW4 = {"GGNN": dict(message_size=3, gather_width=2, enn_hidden_dim=3, mlp1_hidden_dim=1, mlp2_hidden_dim=2),
          "AttGGNN": dict(message_size=3, gather_width=2, msg_hidden_dim=3, att_hidden_dim=3, mlp1_hidden_dim=1,
                          mlp2_hidden_dim=2),
          "MNN": dict(message_size=3, mlp1_hidden_dim=1, mlp2_hidden_dim=2)}


def config(model, over):
    g = (GDB13["n_atom_types"], GDB13["n_formal_charge"], GDB13["max_n_nodes"])
    return MO.mnn_config(*g, **over) if model == "MNN" else O.shaped_config(*g, **over)


def case(name, B=420, seed=61):
    model, over = CASES[name]
    return model, config(model, over), synthetic.make_batch(B, **GDB13, seed=seed)


def init(model, cfg, seed=31):
    return MO.init_params(cfg, seed=seed) if model == "MNN" else O.init_params(cfg, seed=seed, model=model)


def make(model, cfg, P):
    return build_mnn(cfg, P) if model == "MNN" else build(model, cfg, P)


def run_ggnn_parity(name, model, cfg, n8, e8, a8, modes=MODES, seed=31):
    """The loop of tests/test_depths_gpu.py::test_model_parity_across_depths_and_passes for one case."""
    P = O.init_params(cfg, seed=seed, model=model)
    kind = L.KIND_ATTGGNN if model == "AttGGNN" else L.KIND_GGNN
    lib = L.load()
    was = lib.gi_bf3_enable(-1), lib.gi_x2_enable(-1)
    old_threads = torch.get_num_threads()
    torch.set_num_threads(max(1, min(32, torch.get_num_threads())))
    report = {}
    try:
        for mode in modes:
            _set_mode(lib, mode)
            m = build(model, cfg, P)
            params = list(m.parameters())
            nodes, edges, tgt = to_dev(n8, e8, a8)
            torch.cuda.synchronize()
            lib.gi_prof_enable(1)
            out, tape = mpnn.ggnn_forward_raw(m.constants, nodes, edges, params, kind)
            dims, graph, ws = tape
            signs = pins.signs_from_hip(dims, graph, ws, out, attn=kind == L.KIND_ATTGGNN)
            mask_pin = pins.mask_pin_from_hip(dims, graph, ws, n8.shape[0], cfg["big_positive"])
            g = pins.graph_arrays(graph)
            o_leaf = out.detach().clone().requires_grad_(True)
            loss = O.kl_loss(o_leaf, tgt)
            loss.backward()
            grads, _ = mpnn.ggnn_backward_raw(tape, out, o_leaf.grad, params)
            torch.cuda.synchronize()
            ms = (C.c_double * 2)(); busy = (C.c_double * 2)(); work = (C.c_double * 2)(); nl = (C.c_int * 2)()
            L.check(lib.gi_prof_collect(ms, busy, work, nl), "gi_prof_collect")
            lib.gi_prof_enable(0)
            report[mode] = _pipes(lib)
            check_pipes(name, mode, report[mode], has_wide_layer(cfg))
            names = [k for k, _ in m.named_parameters()]
            assert_parity_with_both_pins(O, P, cfg, model, n8, e8, a8, out, loss, names, grads, signs, g, mask_pin)
    finally:
        lib.gi_prof_enable(0)
        lib.gi_bf3_enable(was[0]); lib.gi_x2_enable(was[1])
        torch.set_num_threads(old_threads)
    print(f"\n[{name}] GEMM-family launches per matrix pipe and mode: {report}")


@pytest.mark.parametrize("name", list(CASES))
def test_model_parity_at_widths_that_are_no_multiple_of_4(name):
    model, cfg, (n8, e8, a8) = case(name)
    assert n8.shape[0] * n8.shape[1] >= 2560
    assert {cfg["hidden_node_features"] & 3, cfg["message_size"] & 3} != {0}
    if model == "MNN":
        run_mnn_parity(name, cfg, n8, e8, a8)
    else:
        assert len(fully_masked_rows(e8)) >= 1                 # (the gather's masked-graph branch is in the batch)
        run_ggnn_parity(name, model, cfg, n8, e8, a8)


@pytest.mark.parametrize("model", ["GGNN", "AttGGNN", "MNN"])
def test_widths_below_one_vector_are_refused_and_width_4_runs(model):
    """Per key (message_size, gather_width, enn / msg / att hidden, mlp1 hidden, mlp2 hidden; the gather stacks' hidden
    widths and hidden_node_features likewise): a width below 4 is a ValueError at construction that names the key — the
    choice for EVERY key, because each of them is the row length of a weight matrix that gi_gemm reads as stored.
    tests/test_limits_cpu.py checks each key on its own; here the issue's combined configuration is refused before
    anything is launched, and the same model with those keys at 4 (the limit itself) meets the parity protocol at
    B = 64 in the fp32 mode."""
    cls = {"GGNN": mpnn.GGNN, "AttGGNN": mpnn.AttentionGGNN, "MNN": mpnn.MNN}[model]
    consts = MO.as_constants if model == "MNN" else O.as_constants
    with pytest.raises(ValueError, match=r"message_size = 3: "):
        cls(consts(dict(config(model, BELOW4[model]), device="cuda")))
    cfg = config(model, MIN4[model])
    n8, e8, a8 = synthetic.make_batch(64, **GDB13, seed=62)
    if model == "MNN":
        lib = L.load()
        was = lib.gi_bf3_enable(-1), lib.gi_x2_enable(-1)
        try:
            _set_mode(lib, "fp32")
            from tests.test_mnn_dims_gpu import assert_mnn_parity, hip_step
            P = MO.init_params(cfg, seed=31)
            out, loss, grads, signs, g, pipes = hip_step(lib, cfg, P, n8, e8, a8)
            check_pipes("min4", "fp32", pipes, False)
            assert_mnn_parity("min4", "fp32", cfg, P, n8, e8, a8, out, loss, grads, signs, g)
        finally:
            lib.gi_prof_enable(0)
            lib.gi_bf3_enable(was[0]); lib.gi_x2_enable(was[1])
    else:
        assert len(fully_masked_rows(e8)) >= 1
        run_ggnn_parity("min4", model, cfg, n8, e8, a8, modes=("fp32",))


@pytest.mark.parametrize("name", ["ggnn_r2_r1", "att_r2_r1", "mnn_r2_r1"])
def test_sync_free_forward_equals_the_ordinary_forward(name):
    """tests/test_syncfree_gpu.py / tests/test_mnn_gpu.py's criterion at odd widths: the bounded forward sizes grids and
    picks launch classes by the bounds, so it agrees with the ordinary one to 1e-5 of the largest logit; two bounded
    forwards agree bit for bit."""
    model, cfg, (n8, e8, _) = case(name)
    m = make(model, cfg, init(model, cfg, seed=3)).eval()
    nodes, edges = to_dev(n8, e8)
    with torch.no_grad():
        ref = m(nodes, edges).clone()
        m.sync_free = True
        out = m(nodes, edges).clone()
        again = m(nodes, edges).clone()
    assert m.last_bounded_error() == 0
    assert bool(torch.isfinite(ref).all())
    assert float((out - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    assert torch.equal(out, again)


@pytest.mark.parametrize("name", ["ggnn_r2_r1", "mnn_r2_r1"])
def test_fused_adam_tracks_oracle_adam_with_unaligned_bucket_segments(name):
    """tests/test_mnn_gpu.py::test_fused_adam_tracks_oracle_adam's criterion, five steps on 48 graphs: FusedAdam walks
    the flat gradient bucket, whose segments are padded to 4 floats — at these widths most are no multiple of 4 long
    (50 x 37 weights, 150-float biases ...)."""
    from graphinvent_amd.optim import FusedAdam
    model, cfg, _ = case(name, B=1)
    n8, e8, a8 = synthetic.make_batch(48, **GDB13, seed=63, frac_empty=0.0, frac_single=0.0)
    P = init(model, cfg, seed=4)
    assert sum((v.numel() & 3) != 0 for v in P.values()) >= len(P) // 2   # (unaligned segment ends in the bucket)
    m = make(model, cfg, P).train()
    steps, lr = 5, 1e-3
    opt = FusedAdam(m.parameters(), lr=lr)
    leaves = [P[k].clone().double().requires_grad_(True) for k in P]
    ref_opt = torch.optim.Adam(leaves, lr=lr)
    nodes, edges, tgt = to_dev(n8, e8, a8)
    n64, e64, t64 = (torch.from_numpy(x).double() for x in (n8, e8, a8))
    fwd = MO.mnn_forward if model == "MNN" else O.FORWARDS[model]
    for _ in range(steps):
        m.zero_grad(set_to_none=True)
        O.kl_loss(m(nodes, edges), tgt).backward()
        opt.step()
        ref_opt.zero_grad()
        O.kl_loss(fwd(dict(zip(P, leaves)), cfg, n64, e64), t64).backward()
        ref_opt.step()
    torch.cuda.synchronize()
    for (k, p), r in zip(m.named_parameters(), leaves):
        diff = p.detach().cpu().double() - r.detach()
        assert float(diff.abs().max()) <= 2 * lr * steps, k
        if r.numel() >= 1000:
            assert float(diff.norm() / r.detach().norm().clamp_min(1e-12)) < 5e-4, k


def _profiled_launches(model, cfg, P, n8, e8, a8):
    """gi_prof_collect's launch counts (GEMM family, segmented sums) of one training forward and of its backward."""
    lib = L.load()
    m = build(model, cfg, P)
    params = list(m.parameters())
    nodes, edges, tgt = to_dev(n8, e8, a8)

    def collect():
        torch.cuda.synchronize()
        ms = (C.c_double * 2)(); busy = (C.c_double * 2)(); work = (C.c_double * 2)(); nl = (C.c_int * 2)()
        L.check(lib.gi_prof_collect(ms, busy, work, nl), "gi_prof_collect")
        return nl[0], nl[1]
    torch.cuda.synchronize()
    lib.gi_prof_enable(1)
    try:
        out, tape = mpnn.ggnn_forward_raw(m.constants, nodes, edges, params, m._KIND)
        fwd = collect()
        o_leaf = out.detach().clone().requires_grad_(True)
        O.kl_loss(o_leaf, tgt).backward()
        mpnn.ggnn_backward_raw(tape, out, o_leaf.grad, params)
        bwd = collect()
    finally:
        lib.gi_prof_enable(0)
    return dict(forward=dict(gemm=fwd[0], seg=fwd[1]), backward=dict(gemm=bwd[0], seg=bwd[1]))


def test_odd_widths_take_the_unfused_branches():
    """ggnn_r2_r1 (H 50 / M 37) against the same model at H 48 / M 36, same batch, 3 passes, fp32 mode.  What the
    driver's branches imply for the launches gi_prof_collect counts: the GRU forward fallback is one grouped GEMM launch
    where the fused kernel was one (the scalar gate kernel is not a profiled class), so the forward's GEMM-family count
    cannot drop; the backward loses the folded d h scatter and makes one gi_seg_sum launch per pass after the first
    instead — at least passes - 1 = 2 segmented-sum launches more, and no fewer GEMM-family launches."""
    n8, e8, a8 = synthetic.make_batch(420, **GDB13, seed=61)
    lib = L.load()
    was = lib.gi_bf3_enable(-1), lib.gi_x2_enable(-1)
    counts = {}
    try:
        _set_mode(lib, "fp32")
        for tag, hm in (("H50_M37", {}), ("H48_M36", dict(hidden_node_features=48, message_size=36))):
            cfg = config("GGNN", dict(CASES["ggnn_r2_r1"][1], **hm))
            assert cfg["message_passes"] == 3
            counts[tag] = _profiled_launches("GGNN", cfg, O.init_params(cfg, seed=33), n8, e8, a8)
    finally:
        lib.gi_bf3_enable(was[0]); lib.gi_x2_enable(was[1])
    print(f"\n[GGNN] launches by gi_prof_collect class, odd against multiple-of-4 widths: {counts}")
    odd, even = counts["H50_M37"], counts["H48_M36"]
    assert odd["backward"]["seg"] >= even["backward"]["seg"] + 2, counts
    assert odd["forward"]["gemm"] >= even["forward"]["gemm"] and odd["backward"]["gemm"] >= even["backward"]["gemm"], counts
    total = lambda c: sum(c["forward"].values()) + sum(c["backward"].values())
    assert total(odd) > total(even), counts
