"""-m gpu: model-level parity across MLP depths and message-pass counts (the axis tests/test_dims_gpu.py leaves).

Every other model test runs stacks 2 to 4 deep with 2 or 3 passes.  The reference accepts any depth and pass count
(parameters/defaults.py: enn_depth, msg_depth, att_depth, gather_*_depth, mlp*_depth, message_passes), and the driver
(csrc/gi_model.hip) branches on both:

  depth0        every stack one Linear: first layer = last layer (pass-0 class rows produce the messages directly, the
                last layer's in-place dZ is the input-gradient layer, the graph-level stacks are one split-K layer)
  depth1        one hidden activation per stack
  mixed         enn 0, gather_att 1, gather_emb 3, mlp1 0, mlp2 1
  chain_maxl    enn_depth 7 = 8 Linear layers = GI_CHAIN_MAXL: the chain kernels at their layer limit, 5 passes
  chain_over    enn_depth 8: the message stacks no longer fit a chain and run layer by layer
  passes1       pass 0 is also the last pass (class rows, one-slab weight gradients, no amax cells)
  passes0       no message stack and no GRU run; the readout reads hx[0]; their gradients are None (module path)
  att_m0_a8_p1  AttentionGGNN, msg 0 / att 8, 1 pass: the message family on the chain, the energy family layer by layer
  att_m7_a0     AttentionGGNN, msg 7 / att 0
  att_p0        AttentionGGNN, 0 passes
  deep11_p2     every stack 11 deep (12 Linear layers), 2 passes, narrow widths: 244 parameter tensors, past the 160 the
                backward's slab plan and reduction lists used to hold
  deepest       the same stacks and 16 passes: the driver's own limits.  This model is ill-conditioned in fp32 (the
                oracle's own fp32 logits differ from its fp64 ones by 7e-4, its gradients by 3e-2 as one vector and up
                to ~1e-2 in single tensors), so it is held against the fp64 oracle instead: see its test

Protocol = tests/test_dims_gpu.py: logits, loss and every gradient tensor at 1e-4 against the fp32 oracle's autograd
with the SELU branches and masked-graph energy quanta pinned to the HIP forward's, live rows also against the plain
oracle, in the three arithmetic modes, `gi_prof_pipes` showing the pipes each mode took; GDB-13-shaped batches of
420 graphs (> 2 560 node rows), fully-masked graphs included.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from graphinvent_amd import lib as L, synthetic
from graphinvent_amd.gnn import mpnn
from oracle import ggnn_oracle as O
from tests import pins
from tests.test_dims_gpu import MODES, _pipes, _set_mode
from tests.test_model_gpu import assert_parity_with_both_pins, fully_masked_rows, to_dev

pytestmark = pytest.mark.gpu

GGNN_DEPTHS = ("enn_depth", "gather_att_depth", "gather_emb_depth", "mlp1_depth", "mlp2_depth")
ATT_DEPTHS = ("msg_depth", "att_depth") + GGNN_DEPTHS[1:]

#: name -> (model, overrides of the GDB-13 default config)
CASES = {
    "depth0": ("GGNN", {k: 0 for k in GGNN_DEPTHS}),
    "depth1": ("GGNN", {k: 1 for k in GGNN_DEPTHS}),
    "mixed": ("GGNN", dict(enn_depth=0, gather_att_depth=1, gather_emb_depth=3, mlp1_depth=0, mlp2_depth=1)),
    "chain_maxl": ("GGNN", dict(enn_depth=7, message_passes=5)),
    "chain_over": ("GGNN", dict(enn_depth=8)),
    "passes1": ("GGNN", dict(message_passes=1)),
    "passes0": ("GGNN", dict(message_passes=0)),
    "att_m0_a8_p1": ("AttGGNN", dict(msg_depth=0, att_depth=8, message_passes=1)),
    "att_m7_a0": ("AttGGNN", dict(msg_depth=7, att_depth=0)),
    "att_p0": ("AttGGNN", dict(message_passes=0)),
}
#: every stack at the depth limit, narrow widths (the oracle stays cheap), mlp1 wide enough for the 16-bit pipes
DEEP = dict({k: L.MODEL_MAX_DEPTH for k in GGNN_DEPTHS}, hidden_node_features=32, message_size=32, enn_hidden_dim=48,
            gather_width=32, gather_att_hidden_dim=48, gather_emb_hidden_dim=48, mlp1_hidden_dim=256, mlp2_hidden_dim=64)
CASES["deep11_p2"] = ("GGNN", dict(DEEP, message_passes=2))
DEEPEST = {"deepest": ("GGNN", dict(DEEP, message_passes=L.MODEL_MAX_PASSES))}


def has_wide_layer(cfg) -> bool:
    """A node-level readout / gather layer with both dimensions >= 192 (csrc/gi_model.hip bf3_wide): a hidden-to-hidden
    layer of a stack at least 2 deep — the launches that take the 16-bit pipes at >= 2 560 rows."""
    return any(cfg[d] >= 2 and cfg[h] >= 192 for d, h in (("gather_att_depth", "gather_att_hidden_dim"),
                                                         ("gather_emb_depth", "gather_emb_hidden_dim"),
                                                         ("mlp1_depth", "mlp1_hidden_dim")))


def check_pipes(name, mode, n, wide):
    """test_dims_gpu's pipe check; the 16-bit pipes are required only where the case has a layer wide enough."""
    assert n["fp32"] > 0, (name, mode, n)
    if mode == "fp32":
        assert n["bf16x3"] == 0 and n["fp16x2"] == 0, (name, mode, n)
    elif mode == "bf16x3":
        assert n["fp16x2"] == 0 and (n["bf16x3"] > 0 or not wide), (name, mode, n)
    else:
        assert n["fp16x2"] > 0 or not wide, (name, mode, n)


def case(name, B=420, seed=41):
    model, over = {**CASES, **DEEPEST}[name]
    sh = synthetic.SHAPES["gdb13"]
    cfg = O.shaped_config(sh["n_atom_types"], sh["n_formal_charge"], sh["max_n_nodes"], **over)
    return model, cfg, synthetic.make_batch(B, **sh, seed=seed)


def build(model, cfg, P):
    cls = mpnn.AttentionGGNN if model == "AttGGNN" else mpnn.GGNN
    m = cls(O.as_constants(dict(cfg, device="cuda")))
    m.load_state_dict(P)
    return m.to("cuda")


def launches(model, cfg, P, n8, e8, a8):
    """GEMM-family launches (GEMMs and chains) of one training forward and of its backward."""
    lib = L.load()
    m = build(model, cfg, P)
    params = list(m.parameters())
    nodes, edges, tgt = to_dev(n8, e8, a8)

    def collect():
        torch.cuda.synchronize()
        ms = (C.c_double * 2)(); busy = (C.c_double * 2)(); work = (C.c_double * 2)(); nl = (C.c_int * 2)()
        L.check(lib.gi_prof_collect(ms, busy, work, nl), "gi_prof_collect")
        return nl[0]
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
    return fwd, bwd


@pytest.mark.parametrize("name", list(CASES))
def test_model_parity_across_depths_and_passes(name):
    model, cfg, (n8, e8, a8) = case(name)
    assert n8.shape[0] * n8.shape[1] >= 2560 and len(fully_masked_rows(e8)) >= 1
    P = O.init_params(cfg, seed=31, model=model)
    if name == "deep11_p2":
        assert len(P) > 160                                  # (the parameter-table size the driver used to stop at)
    kind = L.KIND_ATTGGNN if model == "AttGGNN" else L.KIND_GGNN
    lib = L.load()
    was = lib.gi_bf3_enable(-1), lib.gi_x2_enable(-1)
    old_threads = torch.get_num_threads()
    torch.set_num_threads(max(1, min(32, torch.get_num_threads())))
    report = {}
    try:
        for mode in MODES:
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


@pytest.mark.parametrize("name", ["passes0", "att_p0"])
def test_zero_passes_leave_the_message_parameters_without_gradient(name):
    """The reference's .grad of every msg_nns.* / att_nns.* / gru.* parameter stays None at 0 passes (the forward
    never reads them): through loss.backward() on both autograd paths, and an existing .grad is left as it is."""
    model, cfg, (n8, e8, a8) = case(name, B=64)
    P = O.init_params(cfg, seed=32, model=model)
    _, _, g32 = O.forward_backward(P, cfg, *(torch.from_numpy(x).float() for x in (n8, e8, a8)), model=model)
    unused = {k for k, v in g32.items() if v is None}
    assert unused == {k for k in P if k.startswith(("msg_nns.", "att_nns.", "gru."))}
    nodes, edges, tgt = to_dev(n8, e8, a8)
    for autograd_params in (False, True):
        m = build(model, cfg, P)
        m.autograd_params = autograd_params
        O.kl_loss(m(nodes, edges), tgt).backward()
        for k, p in m.named_parameters():
            if k in unused:
                assert p.grad is None, (autograd_params, k)
            else:
                assert p.grad is not None and float((p.grad.cpu() - g32[k]).abs().max()) <= \
                    1e-4 * max(float(g32[k].abs().max()), 1e-30), (autograd_params, k)
        # accumulation: a held gradient of an unused parameter is not touched
        held = {k: torch.full_like(p, 7.0) for k, p in m.named_parameters() if k in unused}
        for k, p in m.named_parameters():
            if k in unused:
                p.grad = held[k].clone()
        O.kl_loss(m(nodes, edges), tgt).backward()
        for k, p in m.named_parameters():
            if k in unused:
                assert torch.equal(p.grad, held[k]), (autograd_params, k)
    # and the optimizer the reference's Workflow builds leaves them where they are
    m = build(model, cfg, P)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-4)
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    O.kl_loss(m(nodes, edges), tgt).backward()
    opt.step()
    for k, p in m.named_parameters():
        assert torch.equal(p.detach(), before[k]) == (k in unused), k


@pytest.mark.parametrize("model", ["GGNN", "AttGGNN"])
def test_message_stacks_take_the_chain_up_to_its_layer_limit(model):
    """At depth 7 (8 layers = GI_CHAIN_MAXL) each pass's stacks of a family are ONE chain launch, forward and dZ
    chain; at depth 8 they run layer by layer (one grouped GEMM per layer).  Same batch, 3 passes: the forward and the
    backward of the deeper model each make at least 6 launches per pass more, while 7 costs (almost) what 6 does — a
    fallback to layer by layer at the limit would add >= 7 launches per pass there.  AttentionGGNN: the energy family's
    depth moves at a fixed msg_depth 7 (msg 7 / att 8: the message family on the chain, the energy family layer by
    layer)."""
    sh = synthetic.SHAPES["gdb13"]
    n8, e8, a8 = synthetic.make_batch(420, **sh, seed=43)
    lib = L.load()
    was = lib.gi_bf3_enable(-1), lib.gi_x2_enable(-1)
    try:
        _set_mode(lib, "fp32")
        counts = {}
        for depth in (6, 7, 8):
            over = dict(msg_depth=7, att_depth=depth) if model == "AttGGNN" else dict(enn_depth=depth)
            cfg = O.shaped_config(sh["n_atom_types"], sh["n_formal_charge"], sh["max_n_nodes"], message_passes=3,
                                  **over)
            counts[depth] = launches(model, cfg, O.init_params(cfg, seed=33, model=model), n8, e8, a8)
    finally:
        lib.gi_bf3_enable(was[0]); lib.gi_x2_enable(was[1])
    print(f"\n[{model}] (forward, backward) GEMM-family launches by depth: {counts}")
    for d in (0, 1):                                          # forward, backward
        assert counts[7][d] - counts[6][d] < 3 * 6, counts   # both on the chain (weight-gradient batches may grow)
        assert counts[8][d] >= counts[7][d] + 3 * 6, counts  # 9 grouped-GEMM layers per pass instead of one chain
    assert counts[7][0] == counts[6][0], counts              # the forward: one chain launch per pass, whatever the depth


def test_chain_pack_and_launch_refuse_a_ninth_layer():
    """gi_mlp_chain_pack / gi_mlp_chain: nlayers > GI_CHAIN_MAXL is GI_ELIMIT (include/graphinvent_amd.h), checked
    before anything is read or launched."""
    lib = L.load()
    p = L.ChainParams()
    p.ngroups, p.rows = 1, 64
    for l in range(L.CHAIN_MAXL):
        p.layer[l].K, p.layer[l].N = 100, 100
    p.nlayers = L.CHAIN_MAXL + 1
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.gi_mlp_chain_pack(C.byref(p), 1, stream) == -2
    assert lib.gi_mlp_chain(C.byref(p), 1, stream) == -2


def test_deepest_model_within_the_fp32_conditioning():
    """Every stack at depth 11 and 16 passes (the driver's limits).  The model is too ill-conditioned for the 1e-4
    protocol: the fp32 oracle's own logits differ from fp64 by 7e-4, its gradients by 3e-2 as one vector and by up to
    ~6e-2 in single tensors, and two correct fp32 evaluations scatter well beyond that ratio (the HIP model measured
    0.17 on a tensor whose fp32-oracle error is 0.016).  So the HIP model is held against the fp64 ORACLE: logits,
    loss and the gradients as one vector within 4x the fp32 oracle's own error (at least 1e-4), and EVERY gradient
    tensor below 0.75 — a zeroed or unreduced tensor (error exactly 1), a sign flip or garbage fails.  Exact parity of
    the same 244-tensor layout is the 1e-4 case deep11_p2.  In the three modes, with the pipes of gi_prof_pipes.  Graphs with every slot masked are left out: their fl32(e - 1e6) energy
    quanta differ between fp32 and fp64 by design (the 1e-4 cases pin them instead)."""
    model, cfg, (n8, e8, a8) = case("deepest")
    live = np.setdiff1d(np.arange(n8.shape[0]), fully_masked_rows(e8))
    n8, e8, a8 = n8[live], e8[live], a8[live]
    assert n8.shape[0] * n8.shape[1] >= 2560
    P = O.init_params(cfg, seed=31, model=model)
    assert len(P) > 160
    t = lambda x, dt: torch.from_numpy(x).to(dt)
    old_threads = torch.get_num_threads()
    torch.set_num_threads(max(1, min(32, torch.get_num_threads())))
    try:
        o32, l32, g32 = O.forward_backward(P, cfg, t(n8, torch.float32), t(e8, torch.float32), t(a8, torch.float32))
        o64, l64, g64 = O.forward_backward({k: v.double() for k, v in P.items()}, cfg, t(n8, torch.float64),
                                           t(e8, torch.float64), t(a8, torch.float64))
    finally:
        torch.set_num_threads(old_threads)
    rel = lambda a, b: float((a.double().cpu() - b).abs().max() / max(float(b.abs().max()), 1e-30))
    bound = lambda a32, a64: 4 * max(rel(a32, a64), 2.5e-5)
    lib = L.load()
    was = lib.gi_bf3_enable(-1), lib.gi_x2_enable(-1)
    try:
        for mode in MODES:
            _set_mode(lib, mode)
            m = build(model, cfg, P)
            nodes, edges, tgt = to_dev(n8, e8, a8)
            torch.cuda.synchronize()
            lib.gi_prof_enable(1)
            out = m(nodes, edges)
            loss = O.kl_loss(out, tgt)
            loss.backward()
            torch.cuda.synchronize()
            ms = (C.c_double * 2)(); busy = (C.c_double * 2)(); work = (C.c_double * 2)(); nl = (C.c_int * 2)()
            L.check(lib.gi_prof_collect(ms, busy, work, nl), "gi_prof_collect")
            lib.gi_prof_enable(0)
            check_pipes("deepest", mode, _pipes(lib), has_wide_layer(cfg))
            assert rel(out.detach(), o64) < bound(o32, o64), (mode, rel(out.detach(), o64), rel(o32, o64))
            assert abs(float(loss.detach()) - float(l64)) < 4 * max(abs(float(l32) - float(l64)), 1e-6 * float(l64))
            names = [k for k, _ in m.named_parameters()]
            hip = torch.cat([p.grad.detach().double().cpu().flatten() for p in m.parameters()])
            ref64 = torch.cat([g64[k].flatten() for k in names])
            ref32 = torch.cat([g32[k].double().flatten() for k in names])
            l2 = lambda a: float((a - ref64).norm() / ref64.norm())
            assert l2(hip) < 4 * max(l2(ref32), 2.5e-5), (mode, l2(hip), l2(ref32))
            for k, p in m.named_parameters():
                e, own = rel(p.grad, g64[k]), rel(g32[k], g64[k])
                assert e < 0.75, (mode, k, e, own)
    finally:
        lib.gi_prof_enable(0)
        lib.gi_bf3_enable(was[0]); lib.gi_x2_enable(was[1])
