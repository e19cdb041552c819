"""-m gpu: parity of the HIP GGNN (through gnn.mpnn.GGNN and the C ABI) with the reference.

Anchors, strongest first:
  * tests/golden/golden_*.npz — logits / loss / gradients produced by the UNMODIFIED reference;
  * the oracle (CPU restatement, itself pinned to those files) run here on the same inputs;
  * size-independent properties at BASELINE.json's full batch size.
Tolerance: north_star's 1e-4 relative fp32 (max|d| / max|ref| per tensor).  Graphs whose every
slot is masked (empty / single atom) carry the reference's fl32(e - 1e6) energy quantisation
(SURVEY.md §7): for them the reference itself is only self-consistent to ~3e-3, so their logits are
checked against a wider bound and, separately, against an fp64 run.
"""
import copy
import os

import numpy as np
import pytest
import torch

from graphinvent_amd import lib as L, ops, synthetic
from graphinvent_amd.gnn import mpnn
from oracle import ggnn_oracle as O
from tests import pins
from tests import ref_dataflow as D
from tests.golden.spec import TINY, digest, tiny_inputs
from tests.two_call import check_two_call_backward

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def make_model(cfg, P):
    cfg = dict(cfg, device="cuda")
    model = mpnn.GGNN(O.as_constants(cfg))
    model.load_state_dict(P)
    return model.to("cuda")


def to_dev(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).float().to(DEV) for a in arrs]


def fully_masked_rows(e8):
    return np.nonzero(~e8.reshape(e8.shape[0], -1).any(1))[0]


def live_loss(logits, apds, live):
    """Workflow.loss (Workflow.py:850-858) over the graphs that are not fully masked: on those rows the reference's
    golden logits and the HIP logits must give the same loss at 1e-4 (the all-rows loss also carries the masked
    graphs' energy quanta, for which the reference's own fp32 and fp64 runs differ by 3e-3)."""
    t = lambda x: torch.as_tensor(np.asarray(x)).float()
    return float(O.kl_loss(t(logits)[live], t(apds)[live]))


def hip_forward_backward(model, n8, e8, a8):
    nodes, edges, tgt = to_dev(n8, e8, a8)
    model.train()
    out = model(nodes, edges)
    model.zero_grad()
    loss = O.kl_loss(out, tgt)          # Workflow.py:850-858 on device (plain torch ops)
    loss.backward()
    grads = {k: p.grad.detach().cpu() for k, p in model.named_parameters()}
    return out.detach().cpu(), float(loss), grads


# ------------------------------------------------------------------------------------------------
def test_forward_stage_by_stage_tiny():
    """Every intermediate buffer of the fused forward against the CPU dataflow model."""
    cfg = O.make_config(**TINY)
    P = O.init_params(cfg, seed=11)
    n8, e8, _ = tiny_inputs()
    ref_out, tape = D.forward(P, cfg, torch.from_numpy(n8).float(), torch.from_numpy(e8).float(),
                              keep=True)
    model = make_model(cfg, P)
    nodes, edges = to_dev(n8, e8)
    out, (dims, graph, ws) = mpnn.ggnn_forward_raw(model.constants, nodes, edges,
                                                   list(model.parameters()))
    S, E, U = graph.S, graph.E, graph.U
    assert (S, E, U) == (tape["g"]["S"], tape["g"]["E"], tape["g"]["U"]) and U < E
    R, B = S + 1, n8.shape[0]
    H, M, G, Fn = dims.H, dims.M, dims.G, dims.Fn
    view = lambda name, rows, i=0, j=0: ops.ws_view(ws, dims, graph, name, rows, i, j)
    assert graph.D0 == tape["g"]["D0"] > 0
    for p, ps in enumerate(tape["passes"]):
        rows = graph.D0 if ps["p0"] else U              # pass 0 runs on the (class, bond type) rows
        assert ps["p0"] == (p == 0)
        assert rel(view("hx", R, p)[:, :H], ps["h_prev"]) < 1e-5, f"hx[{p}]"
        for l in range(dims.enn_depth):
            want = torch.cat([ps["acts_t"][t][l] for t in range(dims.Fe)], 0)
            assert rel(view("eact", rows, p, l)[:, :dims.enn_hidden], want) < 1e-5, f"eact[{p}][{l}]"
        assert rel(view("m", rows, p)[:, :M], ps["m"]) < 1e-5, f"m[{p}]"
        assert rel(view("agg", R, p)[:, :M], ps["agg"]) < 1e-5, f"agg[{p}]"
    hxP = view("hx", R, dims.passes)
    assert rel(hxP[:, :H], tape["h"]) < 1e-5
    assert rel(hxP[:, H:H + Fn], tape["x"]) == 0.0
    assert float(hxP[S].abs().max()) == 0.0
    assert rel(view("en", R)[:, :G], tape["att_acts"][-1]) < 1e-5
    assert rel(view("emb", R)[:, :G], tape["emb_acts"][-1]) < 1e-5
    assert rel(view("add1", R)[:, :dims.A], tape["add1"][-1]) < 1e-5
    assert rel(view("conn1", R)[:, :dims.C], tape["conn1"][-1]) < 1e-5
    NA, NC = dims.N * dims.A, dims.N * dims.C
    assert rel(view("cat_add", B)[:, :NA + G], tape["cat_add"]) < 1e-3      # contains masked graphs
    live = np.setdiff1d(np.arange(B), fully_masked_rows(e8))
    assert rel(view("gemb", B)[live, :G], tape["gemb"][live]) < 1e-5
    assert rel(view("cat_conn", B)[live, :NC + G], tape["cat_conn"][live]) < 1e-5
    assert rel(out[live], ref_out[live]) < 1e-5
    assert rel(out, ref_out) < 5e-3


def test_golden_tiny_logits_loss_grads(golden_dir):
    g = np.load(os.path.join(golden_dir, "golden_tiny.npz"))
    cfg = O.make_config(**TINY)
    P = {k[6:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("param.")}
    model = make_model(cfg, P)
    out, loss, grads = hip_forward_backward(model, g["nodes"], g["edges"], g["apds"])
    masked = fully_masked_rows(g["edges"])
    live = np.setdiff1d(np.arange(out.shape[0]), masked)
    assert rel(out[live], g["logits"][live]) < TOL
    assert rel(out[masked], g["logits"][masked]) < 5e-3        # the reference's own fp32 run, un-pinned ...
    pins.assert_masked_rows_are_quantum_ties(O, model, cfg, P, g["nodes"], g["edges"], out)   # ... and pinned: 1e-4
    assert abs(loss - float(g["loss"])) < 1e-3 * abs(float(g["loss"]))
    ll = live_loss(g["logits"], g["apds"], live)
    assert abs(live_loss(out, g["apds"], live) - ll) < TOL * abs(ll)      # the reference's own logits, live rows: 1e-4
    # gradients: the masked graphs' quantisation noise feeds every weight, so compare against the
    # reference with the same 1e-4 bar where it holds and report the worst tensor
    worst = max((rel(grads[k], g["grad." + k]), k) for k in grads)
    assert worst[0] < 2e-3, worst


def test_tiny_without_masked_graphs_strict(golden_dir):
    """Same config, fully-masked graphs removed: strict 1e-4 on logits, loss and every gradient
    against the oracle (CPU fp32) and a tighter check against the fp64 oracle."""
    cfg = O.make_config(**TINY)
    P = O.init_params(cfg, seed=11)
    n8, e8, a8 = tiny_inputs()
    keep = np.setdiff1d(np.arange(n8.shape[0]), fully_masked_rows(e8))
    n8, e8, a8 = n8[keep], e8[keep], a8[keep]
    model = make_model(cfg, P)
    out, loss, grads = hip_forward_backward(model, n8, e8, a8)
    t = lambda x, dt: torch.from_numpy(x).to(dt)
    o32, l32, g32 = O.forward_backward(P, cfg, t(n8, torch.float32), t(e8, torch.float32),
                                       t(a8, torch.float32))
    P64 = {k: v.double() for k, v in P.items()}
    o64, l64, g64 = O.forward_backward(P64, cfg, t(n8, torch.float64), t(e8, torch.float64),
                                       t(a8, torch.float64))
    assert rel(out, o32) < TOL and rel(out, o64) < 2e-5
    assert abs(loss - float(l32)) < TOL * abs(float(l32))
    for k in grads:
        assert rel(grads[k], g32[k]) < TOL, k
        assert rel(grads[k], g64[k]) < 5e-5, k


def test_golden_gdb13_default_dims(golden_dir):
    g = np.load(os.path.join(golden_dir, "golden_gdb13.npz"))
    cfg = O.make_config()
    P = O.init_params(cfg, seed=int(g["seed"]))
    model = make_model(cfg, P)
    out, loss, grads = hip_forward_backward(model, g["nodes"], g["edges"], g["apds"])
    masked = fully_masked_rows(g["edges"])
    live = np.setdiff1d(np.arange(out.shape[0]), masked)
    assert rel(out[live], g["logits"][live]) < TOL
    assert rel(out[masked], g["logits"][masked]) < 5e-3
    pins.assert_masked_rows_are_quantum_ties(O, model, cfg, P, g["nodes"], g["edges"], out)
    assert abs(loss - float(g["loss"])) < 1e-3 * abs(float(g["loss"]))
    ll = live_loss(g["logits"], g["apds"], live)
    assert abs(live_loss(out, g["apds"], live) - ll) < TOL * abs(ll)
    for k, v in grads.items():
        d, ref = digest(v), g["gdigest." + k]
        scale = max(np.max(np.abs(ref[2:])), 1e-12)
        assert np.max(np.abs(d[2:] - ref[2:])) / scale < 5e-3, k


@pytest.mark.parametrize("split,rows", [("valid", slice(0, 100)), ("test", slice(0, 100)),
                                        ("train", slice(0, 129))])
def test_fixture_batches_vs_oracle(golden_dir, split, rows):
    """The reference's shipped preprocessed data (BASELINE config 1 plumbing case)."""
    d = np.load(os.path.join(golden_dir, f"gdb13_1K-debug_{split}.npz"))
    n8, e8, a8 = d["nodes"][rows], d["edges"][rows], d["APDs"][rows]
    cfg = O.make_config()
    P = O.init_params(cfg, seed=2)
    model = make_model(cfg, P)
    out, loss, grads = hip_forward_backward(model, n8, e8, a8)
    t = lambda x: torch.from_numpy(x).float()
    o32, l32, g32 = O.forward_backward(P, cfg, t(n8), t(e8), t(a8))
    masked = fully_masked_rows(e8)
    live = np.setdiff1d(np.arange(out.shape[0]), masked)
    assert rel(out[live], o32[live]) < TOL
    assert rel(out[masked], o32[masked]) < 5e-3
    pins.assert_masked_rows_are_quantum_ties(O, model, cfg, P, n8, e8, out)
    assert abs(loss - float(l32)) < 1e-3 * abs(float(l32))
    ll = live_loss(o32, a8, live)
    assert abs(live_loss(out, a8, live) - ll) < TOL * abs(ll)
    # batches with fully-masked graphs: a 1/16 energy-quantisation flip or a SELU sign flip moves
    # single tensors by ~1e-2 of their max in either implementation -> global L2 + gross-error cap
    num = sum(float((grads[k].double() - g32[k].double()).pow(2).sum()) for k in grads)
    den = sum(float(g32[k].double().pow(2).sum()) for k in grads)
    worst = max((rel(grads[k], g32[k]), k) for k in grads)
    print(f"\n[unpinned, shipped {split} rows] gradients vs the fp32 oracle: global L2 {(num / den) ** 0.5:.2e}, worst "
          f"tensor {worst[0]:.2e} ({worst[1]})")
    assert (num / den) ** 0.5 < 5e-3, (num / den) ** 0.5
    assert worst[0] < 3e-2, worst


def _live_only(n8, e8, a8):
    keep = np.setdiff1d(np.arange(n8.shape[0]), fully_masked_rows(e8))
    return n8[keep], e8[keep], a8[keep]


#: cap on the worst single gradient tensor (max |d| / max |ref| against fp64) WITHOUT the SELU-branch pin, per shape:
#: a few times what the runs of round 4 printed (the fp32 oracle's own worst tensor is printed beside it and is of
#: the same size: one activation on the other side of the kink moves a 3-output stack by ~1e-2)
UNPINNED_WORST = {"gdb13": 2e-2, "zinc": 2e-2}
#: ... beyond which (up to this) the test must PROVE that the tensor moved because of ties at the SELU kink and nothing
#: else: the same batch differentiated by the fp32 oracle on the branches the HIP forward took (tests/pins.py — which
#: itself asserts that every activation whose branch the pin changes has |pre-activation| < 1e-5 in the oracle's own
#: run) must then agree with the HIP gradients at 1e-4 on EVERY tensor.  (Round 4 had raised the zinc cap to 5e-2 with
#: the fp16x2 chains — 2.06e-2, "a different tie at the kink" — without asserting that; round-4 verdict, weak #2.)
UNPINNED_HARD_CAP = 5e-2


def _oracle_both(cfg, P, n8, e8, a8):
    t = lambda x, dt: torch.from_numpy(x).to(dt)
    r32 = O.forward_backward(P, cfg, t(n8, torch.float32), t(e8, torch.float32), t(a8, torch.float32))
    P64 = {k: v.double() for k, v in P.items()}
    r64 = O.forward_backward(P64, cfg, t(n8, torch.float64), t(e8, torch.float64), t(a8, torch.float64))
    return r32, r64


@pytest.mark.parametrize("shape,B,over", [
    ("gdb13", 1000, dict(hidden_node_features=128, message_size=128)),      # BASELINE config 2
    ("zinc", 96, {}),                                                        # config 3 shape
])
def test_full_size_parity_vs_fp32_and_fp64_oracle(shape, B, over):
    """Logits and loss: strict 1e-4 against the fp32 oracle.  Gradients: the reference's own fp32
    gradients are NOT reproducible to 1e-4 at this size — SELU' is discontinuous at 0 and a few of
    the ~1e7 activations per step round to opposite sides of 0 in fp32 vs fp64 (measured: 4 sign
    flips at B=300 move the fp32 oracle's gradients by up to 5.6e-3 of max|g| from its fp64 run).
    So the raw gradient check is an absolute one — global relative L2 distance from the exact (fp64)
    gradient below 5e-3 for HIP and for the reference's fp32 arithmetic alike, both printed — and a
    per-shape cap on the worst single tensor; the branch-pinned tests below are the strict ones."""
    sh = synthetic.SHAPES[shape]
    cfg = O.shaped_config(sh["n_atom_types"], sh["n_formal_charge"], sh["max_n_nodes"], **over)
    P = O.init_params(cfg, seed=4)
    n8, e8, a8 = _live_only(*synthetic.make_batch(B, **sh, seed=6))
    model = make_model(cfg, P)
    out, loss, grads = hip_forward_backward(model, n8, e8, a8)
    (o32, l32, g32), (o64, l64, g64) = _oracle_both(cfg, P, n8, e8, a8)
    assert rel(out, o32) < TOL and rel(out, o64) < TOL
    assert abs(loss - float(l32)) < TOL * abs(float(l32))
    # raw gradients: global relative L2 error against the exact (fp64) gradient, next to the
    # reference-fp32 oracle's own; per-tensor max-norm only as a gross-error cap (a single SELU
    # sign flip moves small tensors like fConnNet1 by ~1e-2 of their max in either implementation)
    def l2(ga):
        num = sum(float((ga[k].double().cpu() - g64[k]).pow(2).sum()) for k in g64)
        den = sum(float(g64[k].pow(2).sum()) for k in g64)
        return (num / den) ** 0.5
    # (how far a handful of sign flips moves the raw gradients depends on WHICH activations sit at
    # the kink — it changes with every change of summation order, in the reference as in here; the
    # bound is the absolute one, the strict statement is the branch-pinned test below)
    hip_l2, ref_l2 = l2(grads), l2(g32)
    worst = max((rel(grads[k], g64[k]), k) for k in g64)
    worst_ref = max((rel(g32[k], g64[k]), k) for k in g64)
    print(f"\n[unpinned, {shape} B={B}] global L2 vs fp64: HIP {hip_l2:.2e}, fp32 oracle {ref_l2:.2e}; worst tensor: "
          f"HIP {worst[0]:.2e} ({worst[1]}), fp32 oracle {worst_ref[0]:.2e} ({worst_ref[1]})")
    assert hip_l2 < 5e-3 and ref_l2 < 5e-3, (hip_l2, ref_l2)
    assert worst[0] < UNPINNED_HARD_CAP, worst
    if worst[0] >= UNPINNED_WORST[shape]:
        params = list(model.parameters())
        nodes, edges, tgt = to_dev(n8, e8, a8)
        out2, tape = mpnn.ggnn_forward_raw(model.constants, nodes, edges, params)
        dims, graph, ws = tape
        signs = pins.signs_from_hip(dims, graph, ws, out2, attn=False)
        garr = pins.graph_arrays(graph)
        o_leaf = out2.detach().clone().requires_grad_(True)
        O.kl_loss(o_leaf, tgt).backward()
        g_hip, _ = mpnn.ggnn_backward_raw(tape, out2, o_leaf.grad, params)
        t = lambda x: torch.from_numpy(x).float()
        _, _, g_pin, flipped, total = pins.oracle_pinned(O, P, cfg, t(n8), t(e8), t(a8), signs, garr, "GGNN")
        names = [k for k, _ in model.named_parameters()]
        worst_pinned = max((rel(gr, g_pin[k]), k) for k, gr in zip(names, g_hip))
        print(f"[unpinned, {shape}] worst tensor {worst[0]:.2e} >= {UNPINNED_WORST[shape]:.0e}: with the {flipped} of {total} "
              f"tie activations pinned the worst tensor is {worst_pinned[0]:.2e} ({worst_pinned[1]})")
        assert flipped > 0 and flipped < 1e-6 * total, (flipped, total)
        assert worst_pinned[0] < TOL, worst_pinned


@pytest.mark.parametrize("shape,B,over", [
    ("gdb13", 256, dict(hidden_node_features=128, message_size=128)),       # BASELINE config 2 dims
    ("zinc", 64, {}),                                                        # config 3 dims
])
def test_gradients_strict_with_selu_branch_pinned(shape, B, over):
    """Strict 1e-4 gradient parity at BASELINE dimensions: the fp64 dataflow model differentiates
    the same piecewise-smooth branch the HIP forward took (SELU sign pattern read back from the
    HIP activations), which removes the only discontinuity of the loss."""
    sh = synthetic.SHAPES[shape]
    cfg = O.shaped_config(sh["n_atom_types"], sh["n_formal_charge"], sh["max_n_nodes"], **over)
    P = O.init_params(cfg, seed=4)
    n8, e8, a8 = _live_only(*synthetic.make_batch(B, **sh, seed=12))
    model = make_model(cfg, P)
    params = list(model.parameters())
    nodes, edges, tgt = to_dev(n8, e8, a8)
    out, tape_hip = mpnn.ggnn_forward_raw(model.constants, nodes, edges, params)
    dims, graph, ws = tape_hip
    S, E, U, B = graph.S, graph.E, graph.U, n8.shape[0]
    R = S + 1
    view = lambda name, rows, i=0, j=0: ops.ws_view(ws, dims, graph, name, rows, i, j).cpu()
    # fp64 reference forward on the CPU dataflow model
    P64 = {k: v.double() for k, v in P.items()}
    t64 = lambda x: torch.from_numpy(x).double()
    out64, tape = D.forward(P64, cfg, t64(n8), t64(e8), keep=True)
    assert rel(out, out64) < TOL
    pins = {}
    for p, ps in enumerate(tape["passes"]):
        rows = graph.D0 if ps["p0"] else U
        toff = (graph.type_off0 if ps["p0"] else graph.type_off).cpu().tolist()
        for l in range(dims.enn_depth):
            hv = view("eact", rows, p, l)
            for t in range(dims.Fe):
                a = ps["acts_t"][t][l]
                pins[id(a)] = hv[toff[t]:toff[t + 1], :a.shape[1]] > 0
        pins[id(ps["m"])] = view("m", rows, p)[:, :dims.M] > 0
    for key, act_name, out_name, depth in (("att_acts", "att_act", "en", dims.att_depth),
                                           ("emb_acts", "emb_act", "emb", dims.emb_depth),
                                           ("add1", "add1_act", "add1", dims.mlp1_depth),
                                           ("conn1", "conn1_act", "conn1", dims.mlp1_depth)):
        for l in range(depth):
            a = tape[key][l]
            pins[id(a)] = view(act_name, R, 0, l)[:, :a.shape[1]] > 0
        a = tape[key][-1]
        pins[id(a)] = view(out_name, R)[:, :a.shape[1]] > 0
    NA, NC = dims.N * dims.A, dims.N * dims.C
    o_cpu = out.cpu()
    for key, act_name, cols in (("add2", "add2_act", slice(0, NA)),
                                ("conn2", "conn2_act", slice(NA, NA + NC)),
                                ("term2", "term2_act", slice(NA + NC, NA + NC + 1))):
        for l in range(dims.mlp2_depth):
            a = tape[key][l]
            pins[id(a)] = view(act_name, B, 0, l)[:, :a.shape[1]] > 0
        pins[id(tape[key][-1])] = o_cpu[:, cols] > 0
    # backward on both sides
    o_leaf = out.detach().clone().requires_grad_(True)
    O.kl_loss(o_leaf, tgt).backward()
    grads, _ = mpnn.ggnn_backward_raw(tape_hip, out, o_leaf.grad, params)
    o64_leaf = out64.detach().clone().requires_grad_(True)
    O.kl_loss(o64_leaf, t64(a8)).backward()
    D.BRANCH_PINS.clear()
    D.BRANCH_PINS.update(pins)
    try:
        g64 = D.backward(P64, cfg, tape, o64_leaf.grad)
    finally:
        D.BRANCH_PINS.clear()
    names = [k for k, _ in model.named_parameters()]
    for k, g in zip(names, grads):
        assert rel(g, g64[k]) < TOL, k


def assert_parity_with_both_pins(O, P, cfg, model_name, n8, e8, a8, out, loss, names, grads, signs, g, mask_pin):
    """The north_star bar on a batch as the benchmark draws it — ~5 % fully-masked graphs (empty / single atom)
    included: every logit row, the loss and every gradient tensor 1e-4 against the fp32 oracle's own forward +
    autograd with (a) its SELU branches and (b) the fl32(e - 1e6) energy quanta of fully-masked graphs taken
    from the HIP forward (tests/pins.py).  Both pins only break ties: (a) touches < 1e-6 of the activations,
    (b) moves < 1e-3 of the masked graphs' quanta, each by exactly one 1/16 step, with the un-quantised energies
    agreeing to 2e-5.  Rows of graphs that are NOT fully masked also meet 1e-4 against the PLAIN oracle."""
    t = lambda x: torch.from_numpy(x).float()
    o32, l32, g32, flipped, total = pins.oracle_pinned(O, P, cfg, t(n8), t(e8), t(a8), signs, g, model_name,
                                                       mask_pin=mask_pin)
    assert flipped < 1e-6 * total, (flipped, total)
    masked = fully_masked_rows(e8)
    assert mask_pin.graphs == len(masked) and mask_pin.quanta > 0          # the batch does contain them
    assert mask_pin.moved <= 1e-3 * mask_pin.quanta, (mask_pin.moved, mask_pin.quanta)
    assert mask_pin.max_steps <= 1 and mask_pin.max_de < 2e-5, (mask_pin.max_steps, mask_pin.max_de)
    assert rel(out, o32) < TOL                                            # every row, masked graphs included
    assert abs(float(loss) - float(l32)) < TOL * abs(float(l32))
    # a parameter the forward never reads (0 message passes) has no gradient in the oracle: the HIP one is None or 0
    for k, gr in zip(names, grads):
        if g32[k] is None:
            assert gr is None or not bool(gr.any()), k
    worst = max((rel(gr, g32[k]), k) for k, gr in zip(names, grads) if g32[k] is not None)
    assert worst[0] < TOL, worst
    with torch.no_grad():
        plain = O.FORWARDS[model_name](P, cfg, t(n8), t(e8))
    live = np.setdiff1d(np.arange(n8.shape[0]), masked)
    assert rel(out.detach().cpu()[live], plain[live]) < TOL
    return mask_pin.moved


@pytest.fixture
def cpu_threads():
    """The oracle's small GEMMs get SLOWER with hundreds of threads (bench.py: 16 threads 1190
    graphs/s, 256 threads 6)."""
    old = torch.get_num_threads()
    torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))
    yield
    torch.set_num_threads(old)


@pytest.mark.parametrize("shape,B,over", [
    ("gdb13", 1000, dict(hidden_node_features=128, message_size=128)),      # BASELINE configs[1]
    ("zinc", 1000, {}),                                                      # BASELINE configs[2]
])
def test_bench_batch_gradients_1e4_vs_fp32_oracle_autograd(shape, B, over, cpu_threads):
    """The north_star bar on the benchmark's own batches (synthetic.make_batch(B, seed = 1000 rank + i), fully-masked
    graphs included), against the ORACLE ITSELF: see assert_parity_with_both_pins."""
    sh = synthetic.SHAPES[shape]
    cfg = O.shaped_config(sh["n_atom_types"], sh["n_formal_charge"], sh["max_n_nodes"], **over)
    P = O.init_params(cfg, seed=4)
    n8, e8, a8 = synthetic.make_batch(B, **sh, seed=0)          # bench.py's batch 0 of rank 0, as it is
    assert len(fully_masked_rows(e8)) >= B // 50
    model = make_model(cfg, P)
    params = list(model.parameters())
    nodes, edges, tgt = to_dev(n8, e8, a8)
    out, tape_hip = mpnn.ggnn_forward_raw(model.constants, nodes, edges, params)
    dims, graph, ws = tape_hip
    signs = pins.signs_from_hip(dims, graph, ws, out, attn=False)
    mask_pin = pins.mask_pin_from_hip(dims, graph, ws, n8.shape[0], cfg["big_positive"])
    g = pins.graph_arrays(graph)
    o_leaf = out.detach().clone().requires_grad_(True)
    loss = O.kl_loss(o_leaf, tgt)
    loss.backward()
    grads, _ = mpnn.ggnn_backward_raw(tape_hip, out, o_leaf.grad, params)
    names = [k for k, _ in model.named_parameters()]
    assert_parity_with_both_pins(O, P, cfg, "GGNN", n8, e8, a8, out, loss, names, grads, signs, g, mask_pin)


def test_batch_4000_every_16bit_pipe_launch_class_against_the_fp32_mfma_step():
    """bench.py's B = 4000 extra configuration: from 4 000 graphs on the GRAPH-LEVEL stacks' weight gradients run on the
    16-bit pipe too (bf16x3: their operands have no amax cells) beside the node-level ones (fp16x2) — two launch
    classes that must not share a launch (round 4: they did, GI_EINVAL).  Every gradient tensor of the step agrees with
    the same step on the fp32 MFMA alone (gi_bf3_enable(0)) far inside the parity bar, logits and loss likewise."""
    sh = synthetic.SHAPES["gdb13"]
    cfg = O.shaped_config(sh["n_atom_types"], sh["n_formal_charge"], sh["max_n_nodes"], hidden_node_features=128,
                          message_size=128)
    model = make_model(cfg, O.init_params(cfg, seed=4))
    n8, e8, a8 = synthetic.make_batch(4000, **sh, seed=0)
    lib = L.load()
    was = lib.gi_bf3_enable(1)
    try:
        out1, loss1, g1 = hip_forward_backward(model, n8, e8, a8)
        lib.gi_bf3_enable(0)
        out0, loss0, g0 = hip_forward_backward(model, n8, e8, a8)
    finally:
        lib.gi_bf3_enable(was)
    assert rel(out1, out0) < 2e-5 and abs(loss1 - loss0) < 2e-5 * abs(loss0)
    worst = max((rel(g1[k], g0[k]), k) for k in g0)
    print("\nB = 4000: worst gradient tensor against the fp32-MFMA-only step", worst)
    # (SELU ties at the kink flip between two correct fp32 evaluations and move single tensors by up to 5.6e-3 of
    #  max |g| in the reference's own fp32 / fp64 runs; a mis-scaled or missing launch is O(1))
    num = sum(float((g1[k].double() - g0[k].double()).pow(2).sum()) for k in g0)
    den = sum(float(g0[k].double().pow(2).sum()) for k in g0)
    assert worst[0] < 1e-2 and (num / den) ** 0.5 < 1e-3, (worst, (num / den) ** 0.5)


def test_full_batch_properties():
    """BASELINE config 2 at full size incl. masked graphs: run-to-run bit determinism, batch
    permutation equivariance, batch-split consistency, finite outputs."""
    sh = synthetic.SHAPES["gdb13"]
    cfg = O.shaped_config(sh["n_atom_types"], sh["n_formal_charge"], sh["max_n_nodes"],
                          hidden_node_features=128, message_size=128)
    model = make_model(cfg, O.init_params(cfg, seed=8))
    n8, e8, a8 = synthetic.make_batch(1000, **sh, seed=10)
    o1, l1, g1 = hip_forward_backward(model, n8, e8, a8)
    o2, l2, g2 = hip_forward_backward(model, n8, e8, a8)
    assert torch.equal(o1, o2) and l1 == l2
    assert all(torch.equal(g1[k], g2[k]) for k in g1)
    assert bool(torch.isfinite(o1).all()) and all(bool(torch.isfinite(v).all()) for v in g1.values())
    perm = np.random.default_rng(0).permutation(1000)
    op, _, gp = hip_forward_backward(model, n8[perm], e8[perm], a8[perm])
    assert rel(op, o1[perm]) < 1e-5
    # Gradients: the permuted batch sums the weight gradients in another row order (rounding) AND moves a
    # few of the ~1e7 SELU outputs that sit within rounding of 0 to the other side of the kink, each of
    # which changes single gradient entries by O(1) of their size (up to 5.6e-3 of a tensor's
    # max|g| between two correct fp32 evaluations).  So: the gradient as a whole agrees tightly, single
    # tensors within the kink-flip magnitude.  (A fixed 1e-3 per tensor passed / failed — 0.9e-3 .. 1.1e-3 —
    # with ulp-level changes in unrelated kernels.)
    num = sum(float((gp[k].double() - g1[k].double()).pow(2).sum()) for k in g1)
    den = sum(float(g1[k].double().pow(2).sum()) for k in g1)
    assert (num / den) ** 0.5 < 1e-3
    assert max(rel(gp[k], g1[k]) for k in g1) < 1e-2
    model.eval()
    with torch.no_grad():
        halves = [model(*to_dev(n8[s], e8[s])).cpu() for s in (slice(0, 400), slice(400, 1000))]
    assert rel(torch.cat(halves), o1) < 1e-5


def test_module_surface():
    """What the reference's callers do with the model object."""
    cfg = O.make_config(**TINY)
    P = O.init_params(cfg, seed=11)
    model = make_model(cfg, P)
    n8, e8, a8 = tiny_inputs()
    nodes, edges, tgt = to_dev(n8, e8, a8)
    model.eval()
    with torch.no_grad():
        o_eval = model(nodes, edges)
    model.train()
    o_train = model(nodes, edges)
    assert torch.equal(o_eval, o_train) and o_train.requires_grad and not o_eval.requires_grad
    clone = copy.deepcopy(model)                                   # Workflow.py:187-188, 564
    assert torch.equal(clone(nodes, edges), o_train)
    sd = {k: v.cpu() for k, v in model.state_dict().items()}       # Workflow.py:482,498
    assert list(sd) == list(P) and all(torch.equal(sd[k], P[k]) for k in P)
    loss = O.kl_loss(o_train, tgt)
    loss.backward()
    with pytest.raises(RuntimeError):
        O.kl_loss(o_train, tgt).backward()                         # tape already consumed
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    opt.step()                                                     # grads are usable by torch.optim
    assert not torch.equal(model(nodes, edges), o_train)
    with pytest.raises(RuntimeError):
        model(nodes.cpu(), edges.cpu())                            # no CPU fallback


def test_whole_module_pickle_after_a_cuda_forward(tmp_path):
    """``torch.save(model)`` / ``torch.load`` of the MODULE (the reference's v1.0 checkpoints, util.py:841-849) after the
    model has run on the GPU: the fp16x2 guard's pinned host flag, the pass-0 row cache and the other runtime-only state
    stay behind (round-5 advisor: the ctypes pointer made this raise), the copy computes the same logits bit for bit."""
    sh = synthetic.SHAPES["gdb13"]
    cfg = dict(O.shaped_config(sh["n_atom_types"], sh["n_formal_charge"], sh["max_n_nodes"]), device="cuda")
    global CONSTANTS                                   # (pickle looks the constants' class up by module attribute)
    from collections import namedtuple
    CONSTANTS = namedtuple("CONSTANTS", sorted(cfg))
    model = mpnn.GGNN(CONSTANTS(**cfg))
    model.load_state_dict(O.init_params(cfg, seed=2))
    model = model.to("cuda").eval()
    n8, e8, _ = synthetic.make_batch(64, **sh, seed=2)
    nodes, edges = to_dev(n8, e8)
    with torch.no_grad():
        want = model(nodes, edges).clone()
    assert "_x2_guard" in model.__dict__ and model.__dict__["_x2_guard"]
    path = tmp_path / "model.pth"
    torch.save(model, path)
    again = torch.load(path, weights_only=False)
    assert "_x2_guard" not in again.__dict__ and "_p0_state" not in again.__dict__
    with torch.no_grad():
        assert torch.equal(again(nodes, edges), want)
    assert copy.deepcopy(model).__dict__.get("_x2_guard") is None


def test_backward_told_prepacked_without_such_a_forward_packs_itself():
    """GI_BWD_PREPACKED used to be trusted blindly (round-5 advisor): a backward handed the flag for a workspace whose
    forward had NOT packed the W^T / dZ-chain images consumed unwritten memory.  The forward now stamps (workspace,
    arithmetic) into a registry; the backward of an unstamped workspace packs itself: same gradients, bit for bit, as the
    backward of a forward that did prepack."""
    sh = synthetic.SHAPES["gdb13"]
    cfg = O.shaped_config(sh["n_atom_types"], sh["n_formal_charge"], sh["max_n_nodes"], hidden_node_features=128,
                          message_size=128)
    model = make_model(cfg, O.init_params(cfg, seed=3))
    params = list(model.parameters())
    n8, e8, a8 = synthetic.make_batch(500, **sh, seed=9)
    nodes, edges, tgt = to_dev(n8, e8, a8)

    def run(want_backward, lie):
        out, tape = mpnn.ggnn_forward_raw(model.constants, nodes, edges, params, want_backward=want_backward)
        if lie:
            tape[1].run_flags |= L.RUN_PREPACK_BWD                    # the backward will be told "prepacked"
        o_leaf = out.detach().clone().requires_grad_(True)
        O.kl_loss(o_leaf, tgt).backward()
        grads, _ = mpnn.ggnn_backward_raw(tape, out, o_leaf.grad, params)
        torch.cuda.synchronize()
        return [g.clone() for g in grads]

    honest = run(True, False)
    lied = run(False, True)
    assert all(torch.equal(a, b) for a, b in zip(honest, lied))


def test_batch_without_any_edge():
    """Undefined in the reference (GraphGenerator.py:396-423 pins a dummy graph to avoid it);
    defined here: readout only."""
    cfg = O.make_config(**TINY)
    model = make_model(cfg, O.init_params(cfg, seed=11))
    n8, e8, a8 = tiny_inputs()
    e8[:] = 0
    out, loss, grads = hip_forward_backward(model, n8, e8, a8)
    assert bool(torch.isfinite(out).all()) and np.isfinite(loss)
    assert all(float(grads[k].abs().max()) == 0.0 for k in grads if k.startswith(("msg_nns", "gru")))
    assert float(grads["APDReadout.fTermNet2.seq.0.weight"].abs().max()) > 0


def test_training_loop_pieces_on_device(tmp_path):
    """FusedAdam + fused KL loss + DataParallel (nccl group of one rank, collective forced) drive
    the HIP model exactly like torch.optim.Adam + the torch loss expression do."""
    import torch.distributed as dist
    from graphinvent_amd import dp
    from graphinvent_amd.loss import apd_kl_loss, apd_kl_loss_torch
    from graphinvent_amd.optim import FusedAdam
    cfg = O.make_config(**TINY)
    P = O.init_params(cfg, seed=11)
    n8, e8, a8 = _live_only(*tiny_inputs())
    nodes, edges, tgt = to_dev(n8, e8, a8)
    ref_model, model = make_model(cfg, P), make_model(cfg, P)
    ref_opt = torch.optim.Adam(ref_model.parameters(), lr=1e-3)
    own_group = not dist.is_initialized()
    if own_group:
        dist.init_process_group("nccl", init_method=f"file://{tmp_path}/rdzv", rank=0, world_size=1)
    try:
        opt = FusedAdam(model.parameters(), lr=1e-3)
        trainer = dp.DataParallel(model, opt, loss_fn=apd_kl_loss, always_reduce=True)
        trainer.broadcast_parameters()
        for _ in range(3):
            out = ref_model(nodes, edges)
            ref_opt.zero_grad()
            l_ref = apd_kl_loss_torch(out, tgt)
            l_ref.backward()
            ref_opt.step()
            l = trainer.step(nodes, edges, tgt)
            assert trainer.last_bucket_zero_copy            # all-reduce ran in place on the flat bucket
            assert trainer.last_overlapped                  # ... its tail started inside the backward
            assert abs(float(l) - float(l_ref)) < 1e-5 * abs(float(l_ref))
        # Adam divides by sqrt(v): an element whose gradient is ~1e-9 gets an O(lr) update whose
        # sign is decided by rounding noise, so single elements may differ by up to 2*lr per step;
        # the bulk of every tensor must agree.
        for (k, a), b in zip(ref_model.named_parameters(), model.parameters()):
            diff = (b.detach() - a.detach()).double()
            assert float(diff.abs().max()) <= 2 * 1e-3 * 3, k
            # (one noisy element of a 10-element bias is already 1e-3 of its norm)
            bound = 5e-4 if a.numel() >= 1000 else 5e-3
            assert float(diff.norm() / a.detach().double().norm().clamp_min(1e-12)) < bound, k
    finally:
        if own_group:
            dist.destroy_process_group()


def test_int8_inputs_through_the_block_stream_loader(golden_dir):
    """int8 batches (HDF dtype) of the shipped fixture through BlockStreamLoader -> model -> fused loss: the rows are the
    file's rows (bit-exact, tests/test_loader_gpu.py), and logits / loss equal those of the fp32 tensors the
    reference's loader builds from the same rows (BlockDatasetLoader.py:139-141) — checked against the ORACLE on
    those fp32 rows, not only against the HIP model itself."""
    from graphinvent_amd.loader import ArraySource, BlockStreamLoader
    from graphinvent_amd.loss import apd_kl_loss
    d = np.load(os.path.join(golden_dir, "gdb13_1K-debug_train.npz"))
    cfg = O.make_config()
    P = O.init_params(cfg, seed=2)
    model = make_model(cfg, P)
    model.eval()
    loader = BlockStreamLoader(ArraySource(d["nodes"], d["edges"], d["APDs"]), 32, block_size=64, seed=5,
                               drop_last=True)
    assert loader.n_rows == 129 and len(loader) == 4
    n_batches = 0
    with torch.no_grad():
        for nodes, edges, apds in loader:
            assert nodes.is_cuda and nodes.dtype == torch.int8
            out8 = model(nodes, edges)
            out32 = model(nodes.float(), edges.float())
            assert torch.equal(out8, out32)
            l8, l32 = apd_kl_loss(out8, apds), apd_kl_loss(out32, apds.float())
            assert float(l8) == float(l32) and np.isfinite(float(l8))
            o_ref = O.ggnn_forward(P, cfg, nodes.float().cpu(), edges.float().cpu())
            l_ref = O.kl_loss(o_ref, apds.float().cpu())
            live = torch.from_numpy(np.setdiff1d(np.arange(32), fully_masked_rows(edges.cpu().numpy())))
            assert rel(out8.cpu()[live], o_ref[live]) < TOL
            assert abs(float(l8) - float(l_ref)) < 1e-3 * abs(float(l_ref))
            n_batches += 1
    assert n_batches == 4


def test_compaction_prefetched_one_batch_ahead_is_bitwise_identical():
    """ops.prefetch_compact (what the block loader and bench.py call for the NEXT batch) must not
    change a single bit, must be consumed exactly once, and must not be used for a batch that was
    modified after the prefetch."""
    cfg = O.make_config()
    P = O.init_params(cfg, seed=2)
    model = make_model(cfg, P).eval()
    n8, e8, _ = synthetic.make_batch(64, **synthetic.SHAPES["gdb13"], seed=21)
    nodes, edges = to_dev(n8, e8)
    with torch.no_grad():
        ref = model(nodes, edges)
        ops.prefetch_compact(nodes, edges)
        assert len(ops._PREFETCHED) == 1
        assert torch.equal(model(nodes, edges), ref)
        assert len(ops._PREFETCHED) == 0                        # consumed
        ops.prefetch_compact(nodes, edges)
        edges[0, 0, 1, :] = 0; edges[0, 1, 0, :] = 0            # in-place edit -> new tensor version
        out = model(nodes, edges)
        assert len(ops._PREFETCHED) == 1                        # stale entry was NOT used
        ops._PREFETCHED.clear()
        assert torch.equal(out, model(nodes, edges))
        assert not torch.equal(out[0], ref[0])


@pytest.mark.parametrize("passes", [0, 1, 3])
def test_two_call_backward_is_bitwise_the_single_call_backward(passes, monkeypatch):
    """gi_ggnn_backward_phase(READOUT) + (PASSES) — what the overlapped data-parallel exchange uses —
    must give exactly the gradients of the single call, and the hook must see the readout tail.  (1 pass: the
    second phase differentiates pass 0 alone, which is also the last pass; 0 passes: it has nothing to do.)
    With the weight gradients on their side stream and with everything on one stream.  (AttentionGGNN and MNN:
    the tests of the same name in test_attggnn_gpu.py / test_mnn_gpu.py.)"""
    cfg = O.make_config(message_passes=passes)
    P = O.init_params(cfg, seed=2)
    model = make_model(cfg, P)
    params = list(model.parameters())
    n8, e8, a8 = synthetic.make_batch(200, **synthetic.SHAPES["gdb13"], seed=31)
    nodes, edges, tgt = to_dev(n8, e8, a8)
    for side_stream in (True, False):
        monkeypatch.setattr(mpnn, "WGRAD_SIDE_STREAM", side_stream)
        seen = check_two_call_backward(model, L.KIND_GGNN, nodes, edges, tgt)
        names = [k for k, _ in model.named_parameters()]
        first = names.index("gather.att_nn.seq.0.weight")
        assert seen["split"] == sum((p.numel() + 3) & ~3 for p in params[:first])
        assert 0.8 < 1 - seen["split"] / seen["n"] < 0.9           # the tail is most of the bucket


def test_direct_gradient_writeback_has_autograd_accumulate_semantics():
    """Default mode: loss.backward() fills param.grad straight from the fused backward (one autograd
    input instead of 104).  It must behave like the autograd_params=True mode for everything the
    reference's training loops do: same gradients bit for bit, accumulation over several backward
    calls, frozen parameters, zero_grad, no_grad, deepcopy, the second-backward error."""
    cfg = O.make_config(**TINY)
    P = O.init_params(cfg, seed=11)
    n8, e8, a8 = _live_only(*tiny_inputs())
    nodes, edges, tgt = to_dev(n8, e8, a8)
    fast, slow = make_model(cfg, P), make_model(cfg, P)
    slow.autograd_params = True
    for m in (fast, slow):
        O.kl_loss(m(nodes, edges), tgt).backward()
    for (k, a), b in zip(fast.named_parameters(), slow.parameters()):
        assert torch.equal(a.grad, b.grad), k
    bucket = fast._grad_bucket
    assert bucket is not None and all(p.grad.untyped_storage().data_ptr() == bucket.untyped_storage().data_ptr()
                                      for p in fast.parameters())
    # accumulation: a second backward without zero_grad adds, like AccumulateGrad
    g1 = [p.grad.clone() for p in fast.parameters()]
    out = fast(nodes, edges)
    loss = O.kl_loss(out, tgt)
    loss.backward()
    for p, g in zip(fast.parameters(), g1):
        assert rel(p.grad, 2 * g) < 1e-6
    with pytest.raises(RuntimeError):                          # the tape is consumed
        loss.backward()
    # zero_grad -> fresh bucket again, same values as the first time
    fast.zero_grad(set_to_none=True)
    O.kl_loss(fast(nodes, edges), tgt).backward()
    assert all(torch.equal(p.grad, g) for p, g in zip(fast.parameters(), g1))
    # frozen parameters get no gradient; the others are unchanged
    fast.zero_grad(set_to_none=True)
    frozen = fast.gru.weight_hh
    frozen.requires_grad_(False)
    O.kl_loss(fast(nodes, edges), tgt).backward()
    assert frozen.grad is None
    assert all(torch.equal(p.grad, g) for p, g in zip(fast.parameters(), g1) if p is not frozen)
    frozen.requires_grad_(True)
    # no_grad / deepcopy
    with torch.no_grad():
        assert not fast(nodes, edges).requires_grad
    clone = copy.deepcopy(fast)
    clone.zero_grad(set_to_none=True)
    O.kl_loss(clone(nodes, edges), tgt).backward()
    assert all(torch.equal(p.grad, g) for p, g in zip(clone.parameters(), g1))
    assert clone._grad_bucket.data_ptr() != fast._grad_bucket.data_ptr()
    # the full-autograd mode supports torch.autograd.grad on the parameters
    gs = torch.autograd.grad(O.kl_loss(slow(nodes, edges), tgt), list(slow.parameters()))
    assert all(torch.equal(a, b) for a, b in zip(gs, g1))


def test_reinforcement_learning_call_pattern_several_forwards_one_backward():
    """How GraphGeneratorRL drives the model (GraphGeneratorRL.py:131-132, Workflow.py:569-598): in every generation
    round the AGENT runs forward WITH grad and the PRIOR (a deepcopy, Workflow.py:187-188) under no_grad on the same
    graphs; the per-round likelihood terms are combined into one loss and ONE backward runs through all the agent's
    forwards, then the optimizer steps.  Here: three rounds at the default dimensions on batches big enough for the
    16-bit-pipe layers (>= 2 560 node rows), so that three tapes are alive at once — each with its own workspace,
    weight images prepacked on the side stream (GI_RUN_PREPACK_BWD) and amax cells — and are consumed in reverse
    order.  The accumulated gradient must be (a) the sum of the three rounds differentiated one at a time by the same
    kernels, to summation-order noise, (b) the oracle's gradient of the same loss within the unpinned bounds of this
    file; the prior gets no gradient and its forward equals the agent's bit for bit."""
    sh = synthetic.SHAPES["gdb13"]
    cfg = O.shaped_config(sh["n_atom_types"], sh["n_formal_charge"], sh["max_n_nodes"])
    P = O.init_params(cfg, seed=21)
    agent = make_model(cfg, P).train()
    prior = copy.deepcopy(agent).eval()
    rounds = [_live_only(*synthetic.make_batch(420, **sh, seed=70 + k)) for k in range(3)]
    coef = (1.0, 0.5, 2.0)

    def round_term(model, k, with_prior):
        n8, e8, a8 = rounds[k]
        nodes, edges, tgt = to_dev(n8, e8, a8)
        logp = torch.log_softmax(model(nodes, edges), dim=1)
        w = tgt / tgt.sum(1, keepdim=True)
        term = -(w * logp).sum(1)                                   # a likelihood-style per-graph quantity
        if with_prior:
            with torch.no_grad():
                lp_prior = torch.log_softmax(prior(nodes, edges), dim=1)
            term = term + 0.1 * (w * (logp - lp_prior)).sum(1) ** 2
        return coef[k] * term.mean()

    with torch.no_grad():                                           # the copy computes what the original does
        nd, ed = to_dev(rounds[0][0], rounds[0][1])
        assert torch.equal(prior(nd, ed), agent(nd, ed))
    # (a) one backward through three live tapes (a fourth forward's tape is dropped without a backward)
    agent.zero_grad(set_to_none=True)
    loss = sum(round_term(agent, k, True) for k in range(3))
    assert agent(*to_dev(rounds[0][0], rounds[0][1])).requires_grad
    loss.backward()
    torch.cuda.synchronize()
    joint = {k: p.grad.detach().double().cpu() for k, p in agent.named_parameters()}
    assert all(p.grad is None for p in prior.parameters())
    # ... against the rounds differentiated one at a time
    single = {k: torch.zeros_like(v) for k, v in joint.items()}
    for k in range(3):
        agent.zero_grad(set_to_none=True)
        round_term(agent, k, True).backward()
        for name, p in agent.named_parameters():
            single[name] += p.grad.detach().double().cpu()
    for name in joint:
        assert rel(joint[name], single[name]) < 2e-6, name
    # (b) the oracle on the same loss (plain torch autograd on CPU)
    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    total = 0.0
    for k in range(3):
        n8, e8, a8 = rounds[k]
        t = lambda x: torch.from_numpy(x).float()
        logp = torch.log_softmax(O.FORWARDS["GGNN"](Pr, cfg, t(n8), t(e8)), dim=1)
        with torch.no_grad():
            lp_prior = torch.log_softmax(O.FORWARDS["GGNN"](P, cfg, t(n8), t(e8)), dim=1)
        w = t(a8) / t(a8).sum(1, keepdim=True)
        term = -(w * logp).sum(1) + 0.1 * (w * (logp - lp_prior)).sum(1) ** 2
        total = total + coef[k] * term.mean()
    total.backward()
    assert abs(float(loss) - float(total)) < TOL * abs(float(total))
    num = sum(float((joint[k] - Pr[k].grad.double()).pow(2).sum()) for k in joint)
    den = sum(float(Pr[k].grad.double().pow(2).sum()) for k in joint)
    worst = max((rel(joint[k], Pr[k].grad), k) for k in joint)
    print(f"\n[RL pattern] gradients vs the fp32 oracle: global L2 {(num / den) ** 0.5:.2e}, worst tensor {worst[0]:.2e} ({worst[1]})")
    assert (num / den) ** 0.5 < 5e-3 and worst[0] < 3e-2, ((num / den) ** 0.5, worst)
    # the optimizer step the learning step ends with (Workflow.py:598) sees those gradients
    opt = torch.optim.Adam(agent.parameters(), lr=1e-4)
    before = [p.detach().clone() for p in agent.parameters()]
    opt.step()
    assert any(not torch.equal(a, b) for a, b in zip(before, agent.parameters()))


@pytest.mark.parametrize("shape", ["gdb13", "chembl"])
def test_batch_size_extremes_and_row_independence(shape):
    """B = 1 and B = 3 against the oracle; a B = 3000 batch gives every graph the logits it gets in a
    batch of its own third (graphs are independent units: only summation orders may differ)."""
    sh = synthetic.SHAPES[shape]
    cfg = O.shaped_config(sh["n_atom_types"], sh["n_formal_charge"], sh["max_n_nodes"])
    P = O.init_params(cfg, seed=8)
    model = make_model(cfg, P).eval()
    t = lambda x: torch.from_numpy(x).float()
    for B in (1, 3):
        n8, e8, _ = _live_only(*synthetic.make_batch(B + 4, **sh, seed=40 + B))
        n8, e8 = n8[:B], e8[:B]
        with torch.no_grad():
            out = model(*to_dev(n8, e8))
        assert rel(out, O.ggnn_forward(P, cfg, t(n8), t(e8))) < TOL
    Bbig = 3000 if shape == "gdb13" else 600
    n8, e8, a8 = synthetic.make_batch(Bbig, **sh, seed=50)
    nodes, edges, tgt = to_dev(n8, e8, a8)
    model.train()
    out = model(nodes, edges)
    O.kl_loss(out, tgt).backward()
    assert all(bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    third = Bbig // 3
    with torch.no_grad():
        part = model(nodes[third:2 * third].contiguous(), edges[third:2 * third].contiguous())
    live = np.setdiff1d(np.arange(third), fully_masked_rows(e8[third:2 * third]))
    assert rel(out.detach()[third:2 * third][live], part[live]) < 1e-5


@pytest.mark.parametrize("case", ["asymmetric", "real_valued_features", "many_feature_patterns"])
def test_inputs_outside_the_preprocessing_contract(case):
    """Inputs the reference model accepts although DataProcesser never writes them: a directed edge
    from an empty slot, real-valued node features (pass-0 shortcut must switch itself off), and more
    distinct 0/1 feature rows than the pass-0 class table holds (overflow path)."""
    rng = np.random.default_rng(3)
    if case == "asymmetric":
        cfg = O.make_config(**TINY)
        n8, e8, a8 = tiny_inputs()
        n8[4] = 0; e8[4] = 0
        n8[4, 0, 0] = 1; n8[4, 0, 3] = 1
        e8[4, 0, 5, 1] = 1                      # node 0 receives from empty slot 5, nothing back
        nodes_np, expect_p0 = n8.astype(np.float32), True
    else:
        sh = synthetic.SHAPES["zinc"]
        cfg = O.shaped_config(sh["n_atom_types"], sh["n_formal_charge"], sh["max_n_nodes"])
        n8, e8, a8 = _live_only(*synthetic.make_batch(40, **sh, seed=9))
        occupied = n8.any(2)
        if case == "real_valued_features":
            nodes_np = n8.astype(np.float32) * rng.uniform(0.5, 1.5, size=n8.shape).astype(np.float32)
        else:
            nodes_np = (rng.random(n8.shape) < 0.5).astype(np.float32)
            nodes_np[..., 0] = 1.0              # keep occupied slots non-zero
        nodes_np = nodes_np * occupied[..., None]
        expect_p0 = False
    P = O.init_params(cfg, seed=6)
    model = make_model(cfg, P)
    nodes = torch.from_numpy(nodes_np).to(DEV)
    edges, tgt = to_dev(e8, a8)
    out, tape = mpnn.ggnn_forward_raw(model.constants, nodes, edges, list(model.parameters()))
    assert (tape[1].D0 > 0) == expect_p0
    if case == "many_feature_patterns":
        assert len({tuple(r) for r in nodes_np.reshape(-1, nodes_np.shape[2])}) > 256
    ref = O.ggnn_forward(P, cfg, torch.from_numpy(nodes_np), torch.from_numpy(e8).float())
    live = np.setdiff1d(np.arange(out.shape[0]), fully_masked_rows(e8))
    assert rel(out[live], ref[live]) < TOL
    out2 = model(nodes, edges)
    O.kl_loss(out2, tgt).backward()
    leaves = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    O.kl_loss(O.ggnn_forward(leaves, cfg, torch.from_numpy(nodes_np), torch.from_numpy(e8).float()),
              torch.from_numpy(a8).float()).backward()
    num = sum(float((p.grad.cpu().double() - leaves[k].grad.double()).pow(2).sum())
              for k, p in model.named_parameters())
    den = sum(float(v.grad.double().pow(2).sum()) for v in leaves.values())
    assert (num / den) ** 0.5 < 5e-3


@pytest.mark.parametrize("model_name", ["GGNN", "AttGGNN"])
def test_example_training_loop_learns_the_fixture(model_name):
    """examples/train_fixture.py: loader -> model -> fused loss -> FusedAdam on the reference's shipped
    preprocessed data; the training loss must fall clearly (it is a 129-row data set).  "Clearly" is judged on the last
    five epochs together: with the reference's one-cycle schedule (peak lr 1e-3) on 5 steps per epoch the per-epoch loss
    is a noisy, arithmetic-sensitive trajectory — it climbs back to 6-9 around the peak in every arithmetic mode and its
    LAST value alone ranged from 2.4 to 3.9 of an initial 5.96 across the four modes (profiles/r05/fixture_histories.txt)."""
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples",
                        "train_fixture.py")
    spec = importlib.util.spec_from_file_location("train_fixture", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    hist = mod.train(epochs=25, batch=32, model_name=model_name, verbose=False)
    assert all(np.isfinite(hist))
    assert min(hist[-5:]) < 0.6 * hist[0], hist


@pytest.mark.parametrize("model_name", ["GGNN", "AttGGNN"])
def test_four_bond_types_aromatic_preprocessing(model_name):
    """`use_aromatic_bonds` preprocessing gives n_edge_features = 4 (parameters/constants.py:159-166):
    four message MLPs / bond-type groups, logits and loss against the oracle, gradients by global L2."""
    cfg = O.shaped_config(6, 3, 20, n_edge_features=4)
    kind = "AttGGNN" if model_name == "AttGGNN" else "GGNN"
    P = O.init_params(cfg, seed=12, model=kind)
    n8, e8, a8 = _live_only(*synthetic.make_batch(48, 20, 6, 3, n_edge_features=4, seed=77))
    rng = np.random.default_rng(1)                            # make a fifth of the single bonds aromatic
    b, i, j = np.nonzero(np.triu(e8[..., 0], 1))
    pick = rng.random(b.size) < 0.2
    for bb, ii, jj in zip(b[pick], i[pick], j[pick]):
        e8[bb, ii, jj, 0] = e8[bb, jj, ii, 0] = 0
        e8[bb, ii, jj, 3] = e8[bb, jj, ii, 3] = 1
    assert e8.shape[3] == 4 and e8[..., 3].any()
    cls = mpnn.AttentionGGNN if kind == "AttGGNN" else mpnn.GGNN
    model = cls(O.as_constants(dict(cfg, device="cuda")))
    model.load_state_dict(P)
    model = model.to("cuda")
    out, loss, grads = hip_forward_backward(model, n8, e8, a8)
    t = lambda x: torch.from_numpy(x).float()
    o32, l32, g32 = O.forward_backward(P, cfg, t(n8), t(e8), t(a8), model=kind)
    assert rel(out, o32) < TOL
    assert abs(loss - float(l32)) < TOL * abs(float(l32))
    num = sum(float((grads[k].double() - g32[k].double()).pow(2).sum()) for k in grads)
    den = sum(float(g32[k].double().pow(2).sum()) for k in grads)
    assert (num / den) ** 0.5 < 2e-3, (num / den) ** 0.5


def test_multi_bond_pairs_match_the_reference_and_attggnn_refuses_them():
    """The dummy graph of the reference's generation loop (GraphGenerator.py:133, 424-427) carries several bond types on
    one atom pair; the reference's GGNN sums their messages (gnn/mpnn.py:286-294).  HIP GGNN: logits, loss and every
    gradient against the oracle on such a batch; AttentionGGNN, whose neighbour softmax is not defined per bond type
    here, raises instead of computing something else."""
    from tests.test_kernels_gpu import multi_bond_inputs
    n8, e8, a8 = tiny_inputs()
    n8, e8 = multi_bond_inputs(n8, e8)
    cfg = O.make_config(**TINY)
    P = O.init_params(cfg, seed=5)
    model = make_model(cfg, P)
    out, loss, grads = hip_forward_backward(model, n8, e8, a8)
    o_ref, l_ref, g_ref = O.forward_backward(P, cfg, *(torch.from_numpy(x).float() for x in (n8, e8, a8)))
    live = np.setdiff1d(np.arange(n8.shape[0]), fully_masked_rows(e8))
    assert rel(out[live], o_ref[live]) < TOL and abs(loss - float(l_ref)) < 1e-3 * abs(float(l_ref))
    for k in g_ref:
        assert rel(grads[k], g_ref[k]) < 2e-3, k
    with torch.no_grad():                                       # the inference paths: blocking and host-sync-free
        nodes, edges = to_dev(n8, e8)
        model.eval()
        ref = model(nodes, edges)
        model.sync_free = True
        assert torch.equal(model(nodes, edges), ref) and model.last_bounded_error() == 0
    from tests.golden.spec import TINY_ATT
    acfg = dict(O.make_config(**TINY_ATT), device="cuda")
    att = mpnn.AttentionGGNN(O.as_constants(acfg))
    att.load_state_dict(O.init_params(acfg, seed=5, model="AttGGNN"))
    with pytest.raises(ValueError, match="several bond types"):
        att.to("cuda")(nodes, edges)
