"""-m gpu: the MNN model (gnn/mpnn.py:16-74) on the HIP path — its kernels against numpy, the model against the
reference goldens and against the pinned fp32 oracle at B = 1000 in all three arithmetic modes, the readout's dropout
mode, the sync-free forward, FusedAdam and the two-rank data-parallel step."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from graphinvent_amd import lib as L
from graphinvent_amd import ops, synthetic
from graphinvent_amd.gnn import mpnn
from oracle import ggnn_oracle as O
from tests import mnn_oracle as MO
from tests.golden.spec import digest
from tests.two_call import check_two_call_backward
from tests.ref_dataflow import compact

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _i32(x):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.int32))).to(DEV)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _cases(B=24, N=9, seed=4):
    n, e, _ = synthetic.make_batch(B, N, 3, 2, 3, seed=seed, frac_empty=0.1, frac_single=0.1)
    n[0] = 0; e[0] = 0; n[0, 0, 0] = 1; n[0, 0, 3] = 1; e[0, 0, 0, 0] = 1    # dummy self-loop graph
    e[1, 0, 1, :] = 0; e[1, 0, 1, 0] = 1; e[1, 0, 1, 2] = 1                   # a pair with two bond types
    return n, e


# ---- kernels ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["graphs", "no_edges", "nodedup"])
def test_typed_seg_sum_and_transpose(case):
    lib = L.load()
    n, e = _cases()
    if case == "no_edges":
        e[:] = 0
    g = compact(n, e, nodedup=case == "nodedup")
    Fe, H = e.shape[3], 13                                     # (H % 4 != 0: the partial column group)
    R, U = g["S"] + 1, g["U"]
    ldh, lds = 20, ((H * Fe + 3) & ~3) + 4
    rng = np.random.default_rng(1)
    h = rng.standard_normal((R, ldh)).astype(np.float32)
    h[R - 1] = 0.0
    u_type = np.searchsorted(g["type_off"], np.arange(U), side="right") - 1
    ref = MO.typed_sums(h[:, :H].astype(np.float64), g["in_perm"], g["u_src"], u_type, g["seg_off"], Fe)
    hd = torch.from_numpy(h).to(DEV)
    ints = {k: _i32(g[k]) if np.asarray(g[k]).size else torch.zeros(1, dtype=torch.int32, device=DEV)
            for k in ("u_src", "in_perm", "seg_off", "type_off", "out_perm", "src_off", "mu_off", "mu_dst")}
    out = torch.full((R, lds), 7.0, device=DEV)
    L.check(lib.gi_typed_seg_sum(hd.data_ptr(), ldh, ints["u_src"].data_ptr(), ints["in_perm"].data_ptr(),
                                 ints["seg_off"].data_ptr(), ints["type_off"].data_ptr(), R, H, Fe, out.data_ptr(), lds,
                                 _stream()), "gi_typed_seg_sum")
    torch.cuda.synchronize()
    got = out.cpu().double()
    assert (got[:, :H * Fe] - torch.from_numpy(ref)).abs().max() < 1e-5
    assert torch.all(got[:, H * Fe:] == 7.0)                   # nothing written past H * Fe
    has_in = np.diff(g["seg_off"]) > 0
    assert torch.all(got[torch.from_numpy(~has_in), :H * Fe] == 0)   # rows without in-edges (row S among them)
    # transpose, accumulating into a prefilled d h
    dS = rng.standard_normal((R, lds)).astype(np.float32)
    dh0 = rng.standard_normal((R, ldh)).astype(np.float32)
    want = dh0[:, :H].astype(np.float64).copy()
    d3 = dS[:, :H * Fe].reshape(R, H, Fe).astype(np.float64)
    for c in range(R):
        for s in range(g["src_off"][c], g["src_off"][c + 1]):
            u = g["out_perm"][s]
            for k in range(g["mu_off"][u], g["mu_off"][u + 1]):
                want[c] += d3[g["mu_dst"][k], :, u_type[u]]
    dh = torch.from_numpy(dh0).to(DEV)
    L.check(lib.gi_typed_seg_sum_t(torch.from_numpy(dS).to(DEV).data_ptr(), lds, ints["out_perm"].data_ptr(),
                                   ints["src_off"].data_ptr(), ints["mu_off"].data_ptr(), ints["mu_dst"].data_ptr(),
                                   ints["type_off"].data_ptr(), R, H, Fe, dh.data_ptr(), ldh, 1, _stream()),
            "gi_typed_seg_sum_t")
    torch.cuda.synchronize()
    assert (dh.cpu().double()[:, :H] - torch.from_numpy(want)).abs().max() < 1e-5
    assert torch.equal(dh.cpu()[:, H:], torch.from_numpy(dh0[:, H:]))


@pytest.mark.parametrize("nodedup", [False, True])
def test_graph_sum_fwd_bwd(nodedup):
    lib = L.load()
    n, e = _cases()
    B, N = n.shape[:2]
    g = compact(n, e, nodedup=nodedup)
    S, H, ld = g["S"], 10, 12
    R = S + 1
    h = torch.randn(R, ld, device=DEV)
    h[S] = 0
    cidx = _i32(g["cidx"])
    outs = [torch.zeros(B, 16, device=DEV) for _ in range(3)]
    L.check(lib.gi_graph_sum_fwd(h.data_ptr(), ld, cidx.data_ptr(), B, N, H, outs[0].data_ptr() + 4 * 3, 16,
                                 outs[1].data_ptr(), 16, outs[2].data_ptr(), 16, _stream()), "gi_graph_sum_fwd")
    torch.cuda.synchronize()
    ref = h.cpu().double()[torch.from_numpy(g["cidx"].astype(np.int64))].view(B, N, ld)[:, :, :H].sum(1)
    assert rel(outs[0].cpu()[:, 3:3 + H], ref) < 1e-6 and rel(outs[1].cpu()[:, :H], ref) < 1e-6
    assert torch.equal(outs[1], outs[2])
    dg = [torch.randn(B, 12, device=DEV) for _ in range(3)]
    dh = torch.full((R, ld), 3.0, device=DEV)
    L.check(lib.gi_graph_sum_bwd(dg[0].data_ptr(), 12, dg[1].data_ptr(), 12, dg[2].data_ptr(), 12,
                                 _i32(g["slot_of"]).data_ptr(), S, N, H, dh.data_ptr(), ld, 0, _stream()),
            "gi_graph_sum_bwd")
    torch.cuda.synchronize()
    dsum = sum(x.cpu().double() for x in dg)[:, :H]
    want = dsum[torch.from_numpy(g["slot_of"].astype(np.int64) // N)]
    assert (dh.cpu().double()[:S, :H] - want).abs().max() < 1e-6
    assert torch.all(dh.cpu()[S, :H] == 0)                      # the zero row of the padded slots
    assert torch.all(dh.cpu()[:, H:] == 3.0)


# ---- the model ----------------------------------------------------------------------------------------------------
def _model(cfg, P):
    model = mpnn.MNN(MO.as_constants(dict(cfg, device="cuda")))
    model.load_state_dict(P)
    return model.to(DEV).train()


def _step(model, n8, e8, a8):
    nodes, edges, tgt = (torch.from_numpy(x).float().to(DEV) for x in (n8, e8, a8))
    model.zero_grad(set_to_none=True)
    out = model(nodes, edges)
    loss = O.kl_loss(out, tgt)
    loss.backward()
    torch.cuda.synchronize()
    return out.detach().cpu(), float(loss.detach()), {k: p.grad.detach().cpu() for k, p in model.named_parameters()}


@pytest.mark.parametrize("tag", ["", "one."])
def test_tiny_matches_reference_golden(golden_dir, tag):
    g = np.load(os.path.join(golden_dir, "golden_mnn_tiny.npz"))
    cfg = MO.tiny_config()
    P = {k: torch.from_numpy(g["param." + k]) for k in MO.param_shapes(cfg)}
    out, loss, grads = _step(_model(cfg, P), *(g[tag + k] for k in ("nodes", "edges", "apds")))
    assert rel(out, g[tag + "logits"]) < 1e-4
    assert abs(loss - float(g[tag + "loss"])) < 1e-4 * abs(float(g[tag + "loss"]))
    for k, v in grads.items():
        assert rel(v, g[tag + "grad." + k]) < 1e-4, k


def test_gdb13_matches_reference_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "golden_mnn_gdb13.npz"))
    sh = synthetic.SHAPES["gdb13"]
    cfg = MO.mnn_config(sh["n_atom_types"], sh["n_formal_charge"], sh["max_n_nodes"])
    out, loss, grads = _step(_model(cfg, MO.init_params(cfg, seed=int(g["seed"]))),
                             *(g[k] for k in ("nodes", "edges", "apds")))
    assert rel(out, g["logits"]) < 1e-4
    assert abs(loss - float(g["loss"])) < 1e-4 * abs(float(g["loss"]))
    for k, v in grads.items():
        d, ref = digest(v), g["gdigest." + k]
        scale = max(np.max(np.abs(ref[2:])), 1e-12)
        assert np.max(np.abs(d[2:] - ref[2:])) / scale < 2e-3, k      # (SELU kinks: unpinned fp32 vs fp32)
        assert abs(d[1] - ref[1]) <= 2e-3 * ref[1] + 1e-12, k


def mnn_signs(dims, graph, ws, out):
    """SELU-branch pattern of GlobalReadout's stacks of one MNN forward, read through gi_ggnn_ws_query (the MNN
    counterpart of tests/pins.signs_from_hip: no message or gather stacks)."""
    from tests.pins import Signs
    s = Signs()
    R, B = graph.S + 1, out.shape[0]

    def view(name, rows, width, j=0):
        return (ops.ws_view(ws, dims, graph, name, rows, 0, j)[:, :width] > 0).cpu()

    for name, act, last, width in (("APDReadout.fAddNet1", "add1_act", "add1", dims.A),
                                   ("APDReadout.fConnNet1", "conn1_act", "conn1", dims.C)):
        s.node[name] = [view(act, R, dims.mlp1_hidden, l) for l in range(dims.mlp1_depth)] + [view(last, R, width)]
    NA, NC = dims.N * dims.A, dims.N * dims.C
    o = (out > 0).cpu()
    for name, act, cols in (("APDReadout.fAddNet2", "add2_act", slice(0, NA)),
                            ("APDReadout.fConnNet2", "conn2_act", slice(NA, NA + NC)),
                            ("APDReadout.fTermNet2", "term2_act", slice(NA + NC, NA + NC + 1))):
        s.graph[name] = [view(act, B, dims.mlp2_hidden, l) for l in range(dims.mlp2_depth)] + [o[:, cols]]
    return s


MODES = {"fp16x2": (1, 1), "bf16x3": (1, 0), "fp32": (0, 1)}


@pytest.mark.parametrize("mode", list(MODES))
def test_b1000_matches_pinned_oracle(mode):
    from tests.pins import OraclePins, TIE_TOL, graph_arrays
    lib = L.load()
    sh = synthetic.SHAPES["gdb13"]
    cfg = MO.mnn_config(sh["n_atom_types"], sh["n_formal_charge"], sh["max_n_nodes"])
    P = MO.init_params(cfg, seed=5)
    n8, e8, a8 = synthetic.make_batch(1000, **sh, seed=21)
    nodes, edges, tgt = (torch.from_numpy(x).float() for x in (n8, e8, a8))
    params = [P[k].to(DEV).contiguous() for k in MO.param_shapes(cfg)]
    consts = MO.as_constants(dict(cfg, device="cuda"))
    prev = (lib.gi_bf3_enable(MODES[mode][0]), lib.gi_x2_enable(MODES[mode][1]))
    try:
        lib.gi_prof_enable(1)
        out, tape = mpnn.ggnn_forward_raw(consts, nodes.to(DEV), edges.to(DEV), params, L.KIND_MNN)
        signs = mnn_signs(tape[0], tape[1], tape[2], out)
        g = graph_arrays(tape[1])
        leaf = out.detach().clone().requires_grad_(True)
        loss = O.kl_loss(leaf, tgt.to(DEV))
        (d_out,) = torch.autograd.grad(loss, leaf)
        grads, _ = mpnn.ggnn_backward_raw(tape, out, d_out, params)
        torch.cuda.synchronize()
        ms, busy, work, launches = ((ctypes.c_double * 2)(), (ctypes.c_double * 2)(), (ctypes.c_double * 2)(),
                                    (ctypes.c_int * 2)())
        lib.gi_prof_collect(ms, busy, work, launches)
        pm, pw, pl = (ctypes.c_double * 3)(), (ctypes.c_double * 3)(), (ctypes.c_int * 3)()
        lib.gi_prof_pipes(pm, pw, pl)
        lib.gi_prof_enable(0)
    finally:
        lib.gi_bf3_enable(prev[0]); lib.gi_x2_enable(prev[1])
    pipes = list(pl)
    if mode == "fp32":
        assert pipes[0] > 0 and pipes[1] == 0 and pipes[2] == 0, pipes
    elif mode == "bf16x3":
        assert pipes[1] > 0 and pipes[2] == 0, pipes
    else:
        assert pipes[2] > 0, pipes
    pins = OraclePins(signs, g, n8, e8, "MNN")
    O.SELU_BRANCH_HOOK = pins
    try:
        o_ref, l_ref, g_ref = MO.forward_backward(P, cfg, nodes, edges, tgt)
    finally:
        O.SELU_BRANCH_HOOK = None
    assert pins.max_flipped_abs < TIE_TOL and pins.flipped <= 1e-6 * pins.total, (pins.flipped, pins.total)
    assert rel(out, o_ref) < 1e-4
    assert abs(float(loss.detach()) - float(l_ref)) < 1e-4 * abs(float(l_ref))
    for k, gr in zip(MO.param_shapes(cfg), grads):
        assert rel(gr, g_ref[k]) < 1e-4, (k, rel(gr, g_ref[k]))


def test_readout_dropout_matches_oracle_with_hip_masks():
    from tests.dropout_masks import OracleDropout
    cfg = MO.tiny_config(mlp1_dropout_p=0.1, mlp2_dropout_p=0.2)
    P = MO.init_params(cfg, seed=3)
    n8, e8, a8 = synthetic.make_batch(64, 6, 3, 2, 3, seed=8)
    model = _model(cfg, P)
    model.dropout_seed = 12345
    out, loss, grads = _step(model, n8, e8, a8)
    g = compact(n8, e8, nodedup=True)
    # (family_p looks every readout prefix up in one table that also names the gather stacks: MNN has none)
    hook = OracleDropout(dict(cfg, gather_att_dropout_p=0.0, gather_emb_dropout_p=0.0), list(MO.param_shapes(cfg)),
                         12345, g, n8, e8, model="MNN")
    O.DROPOUT_HOOK = hook
    try:
        o_ref, l_ref, g_ref = MO.forward_backward(P, cfg, *(torch.from_numpy(x).float() for x in (n8, e8, a8)))
    finally:
        O.DROPOUT_HOOK = None
    assert hook.sites > 0 and 0 < hook.kept < hook.drawn
    assert rel(out, o_ref) < 1e-4
    assert abs(loss - float(l_ref)) < 1e-4 * abs(float(l_ref))
    for k, v in grads.items():
        assert rel(v, g_ref[k]) < 1e-4, k


@pytest.mark.parametrize("B", [1000, 200])
def test_sync_free_forward_equals_plain_forward(B):
    """Generation-style batch (the dummy self-loop graph with all bond types in slot 0).  The readout's hidden layers
    pick fp32-MFMA or 16-bit-pipe launches by row count — the plain forward by the real rows, the bounded one by the
    bound — so the two agree to fp32 accuracy; two sync-free forwards agree bit for bit."""
    sh = synthetic.SHAPES["gdb13"]
    cfg = MO.mnn_config(sh["n_atom_types"], sh["n_formal_charge"], sh["max_n_nodes"])
    model = _model(cfg, MO.init_params(cfg, seed=2)).eval()
    n8, e8, _ = synthetic.make_batch(B, **sh, seed=6)
    n8[0] = 0; e8[0] = 0; n8[0, 0, 0] = 1; n8[0, 0, sh["n_atom_types"]] = 1; e8[0, 0, 0, :] = 1
    nodes, edges = (torch.from_numpy(x).float().to(DEV) for x in (n8, e8))
    with torch.no_grad():
        plain = model(nodes, edges).clone()
        model.sync_free = True
        free = model(nodes, edges).clone()
        free2 = model(nodes, edges).clone()
    assert model.last_bounded_error() == 0
    assert float((free - plain).abs().max()) <= 1e-5 * float(plain.abs().max())
    assert torch.equal(free, free2)


@pytest.mark.parametrize("side_stream", [True, False])
@pytest.mark.parametrize("passes", [0, 1, 3])
def test_two_call_backward_is_bitwise_the_single_call_backward(passes, side_stream, monkeypatch):
    """gi_ggnn_backward_phase(READOUT) + (PASSES) must give exactly the gradients of the single call (the body of the
    GGNN test of this name in test_model_gpu.py), with the weight gradients on their side stream and on one stream.
    (1 pass: pass 0 is also the last pass; 0 passes: the second phase has nothing to do.)"""
    monkeypatch.setattr(mpnn, "WGRAD_SIDE_STREAM", side_stream)
    sh = synthetic.SHAPES["gdb13"]
    cfg = MO.mnn_config(sh["n_atom_types"], sh["n_formal_charge"], sh["max_n_nodes"], message_passes=passes)
    model = _model(cfg, MO.init_params(cfg, seed=2))
    nodes, edges, tgt = (torch.from_numpy(x).float().to(DEV) for x in synthetic.make_batch(16, **sh, seed=31))
    check_two_call_backward(model, L.KIND_MNN, nodes, edges, tgt)


def test_fused_adam_tracks_oracle_adam():
    from graphinvent_amd.optim import FusedAdam
    cfg = MO.tiny_config()
    P = MO.init_params(cfg, seed=4)
    n8, e8, a8 = synthetic.make_batch(48, 6, 3, 2, 3, seed=9)
    model = _model(cfg, P)
    opt = FusedAdam(model.parameters(), lr=1e-3)
    leaves = [P[k].clone().double().requires_grad_(True) for k in MO.param_shapes(cfg)]
    ref_opt = torch.optim.Adam(leaves, lr=1e-3)
    nodes, edges, tgt = (torch.from_numpy(x) for x in (n8, e8, a8))
    for _ in range(20):
        _step(model, n8, e8, a8)
        opt.step()
        ref_opt.zero_grad()
        Pd = dict(zip(MO.param_shapes(cfg), leaves))
        O.kl_loss(MO.mnn_forward(Pd, cfg, nodes.double(), edges.double()), tgt.double()).backward()
        ref_opt.step()
    # Adam turns a ~0 gradient into an O(lr) step of arbitrary sign: bound single elements by 2 * lr * steps, and
    # the bulk of every sizeable tensor tightly
    for (k, p), r in zip(model.named_parameters(), leaves):
        diff = p.detach().cpu().double() - r.detach()
        assert float(diff.abs().max()) <= 2 * 1e-3 * 20, k
        if r.numel() >= 1000:
            assert float(diff.norm() / r.detach().norm().clamp_min(1e-12)) < 5e-4, k


# ---- data parallel --------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _dp_setup():
    sh = synthetic.SHAPES["gdb13"]
    cfg = MO.mnn_config(sh["n_atom_types"], sh["n_formal_charge"], sh["max_n_nodes"])
    model = _model(cfg, MO.init_params(cfg, seed=7))
    n8, e8, a8 = synthetic.make_batch(64, **sh, seed=3, frac_empty=0.0, frac_single=0.0)
    return model, tuple(torch.from_numpy(x).float().to(DEV) for x in (n8, e8, a8))


def _dp_worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    from graphinvent_amd import dp
    from graphinvent_amd.loss import apd_kl_loss
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    model, (nodes, edges, tgt) = _dp_setup()
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    tr = dp.DataParallel(model, opt, loss_fn=apd_kl_loss, overlap=True)
    sl = slice(32 * rank, 32 * rank + 32)
    tr.step(nodes[sl], edges[sl], tgt[sl])
    torch.save(dict(grads=[p.grad.detach().cpu() for p in model.parameters()], overlapped=tr.last_overlapped),
               os.path.join(out_dir, f"r{rank}.pt"))
    dist.destroy_process_group()


def test_two_ranks_gloo_equal_single_process_gradients(tmp_path):
    from graphinvent_amd.loss import apd_kl_loss
    mp.spawn(_dp_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / f"r{r}.pt") for r in (0, 1))
    assert r0["overlapped"] and r1["overlapped"]
    model, (nodes, edges, tgt) = _dp_setup()
    out = model(nodes, edges)
    apd_kl_loss(out, tgt).backward()
    for (k, p), a, b in zip(model.named_parameters(), r0["grads"], r1["grads"]):
        assert torch.equal(a, b), k
        assert rel(a, p.grad) < 1e-5, k
