"""RL fine-tuning sampling step at the GDB-13 shape (informational; bench.py measures the flagship training workload).

    python tools/bench_rl.py [--batch 1000] [--iters 50] [--warmup 10] [--rounds 8]

Prints one JSON line:
  * sampling_step_us: the step GraphGeneratorRL runs between the model calls and apply_actions, forward + backward of
    sum(wa * agent_like) + sum(wp * prior_like) to both logits tensors — the HIP path (sample_actions_rl) and the
    reference's torch sequence on the same device (tests/rl_callers.py get_actions_rl_torch after two softmaxes);
    hip_fwd = the forward launch alone, hip_fwd_bwd_without_tuples = both launches and autograd without the
    reference-format index tuples (whose boolean-mask gathers read back to the host);
  * round_ms: one RL generation round on the drop-in GGNN (reference defaults): agent forward with grad + prior
    forward with grad + sample_actions_rl;
  * backward_ms: the backward through `rounds` such rounds (both models' tapes), and the forward of those rounds."""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from graphinvent_amd import sampler, synthetic  # noqa: E402
from graphinvent_amd.gnn import mpnn  # noqa: E402
from oracle import ggnn_oracle as O  # noqa: E402
from tests import rl_callers as RL  # noqa: E402


def timed(fn, n, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(n):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=8)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_rl.py needs an MI355X"
    sh = synthetic.SHAPES["gdb13"]
    cfg = O.shaped_config(sh["n_atom_types"], sh["n_formal_charge"], sh["max_n_nodes"])
    N, Fe = cfg["max_n_nodes"], cfg["n_edge_features"]
    dim_f_add = [N, sh["n_atom_types"], sh["n_formal_charge"], Fe]
    dim_f_conn = [N, Fe]
    A = int(np.prod(dim_f_add[1:]))
    W = N * A + N * Fe + 1
    B = a.batch
    n8, e8, _ = synthetic.make_batch(B, **sh, seed=1)
    nodes, edges = (torch.from_numpy(x).float().cuda() for x in (n8, e8))
    n_nodes = (nodes.sum(-1) > 0).sum(-1).to(torch.int8)
    gen = torch.Generator(device="cuda").manual_seed(0)

    # ---- the sampling step alone ------------------------------------------------------------------------------
    la = (torch.randn(B, W, device="cuda", generator=gen) * 2).requires_grad_(True)
    lp = (torch.randn(B, W, device="cuda", generator=gen) * 2).requires_grad_(True)
    wa, wp = torch.randn(B, device="cuda", generator=gen), torch.randn(B, device="cuda", generator=gen)
    sm = torch.nn.Softmax(dim=1)

    def hip_step():
        out = sampler.sample_actions_rl(la, lp, n_nodes, edges, dim_f_add, dim_f_conn, generator=gen)
        torch.autograd.grad((out[4] * wa).sum() + (out[5] * wp).sum(), (la, lp))

    def torch_step():
        out = RL.get_actions_rl_torch(sm(la), sm(lp), n_nodes, edges, dim_f_add, dim_f_conn)
        torch.autograd.grad((out[4] * wa).sum() + (out[5] * wp).sum(), (la, lp))

    def hip_kernels():                       # the two launches and autograd only, without the tuple layout
        out = sampler._SampleRL.apply(la, lp, n_nodes, edges, A, None, gen)
        torch.autograd.grad((out[1] * wa).sum() + (out[2] * wp).sum(), (la, lp))

    def hip_fwd():
        with torch.no_grad():
            sampler.sample_actions_rl_raw(la, lp, n_nodes, edges, A, generator=gen)

    hip_us = timed(hip_step, a.iters, a.warmup) * 1e3
    torch_us = timed(torch_step, a.iters, a.warmup) * 1e3
    hip_fwd_us = timed(hip_fwd, a.iters, a.warmup) * 1e3
    hip_kernels_us = timed(hip_kernels, a.iters, a.warmup) * 1e3
    # bytes the HIP step must move at least: forward reads both rows once; backward reads both rows, writes both
    step_bytes = 2 * B * W * 4 + 2 * (2 * B * W * 4)

    # ---- RL generation rounds on the drop-in GGNN ---------------------------------------------------------------
    P = O.init_params(cfg, seed=0)
    agent = mpnn.GGNN(O.as_constants(dict(cfg, device="cuda")))
    agent.load_state_dict(P)
    agent = agent.cuda().train()
    prior = copy.deepcopy(agent).eval()

    def one_round():
        la_r = agent(nodes, edges)
        lp_r = prior(nodes, edges)
        return sampler.sample_actions_rl(la_r, lp_r, n_nodes, edges, dim_f_add, dim_f_conn, generator=gen)

    def round_only():
        out = one_round()
        del out

    round_ms = timed(round_only, a.iters, a.warmup)

    def rounds_and_backward():
        torch.cuda.synchronize()
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        total = 0
        for _ in range(a.rounds):
            out = one_round()
            total = total + torch.log(out[4]).sum() - torch.log(out[5]).sum()
        e1.record()
        total.backward()
        e2.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), e1.elapsed_time(e2)

    for _ in range(3):
        rounds_and_backward()
    fw, bw = zip(*(rounds_and_backward() for _ in range(max(3, a.iters // 10))))
    print(json.dumps({
        "workload": "rl_sampling", "shape": "gdb13", "batch": B, "W": W, "iters": a.iters, "warmup": a.warmup,
        "sampling_step_us": {"hip_fwd_bwd": round(hip_us, 2), "hip_fwd": round(hip_fwd_us, 2),
                             "hip_fwd_bwd_without_tuples": round(hip_kernels_us, 2),
                             "torch_reference_fwd_bwd": round(torch_us, 2), "speedup": round(torch_us / hip_us, 2)},
        "sampling_step_min_bytes": step_bytes,
        "sampling_step_effective_TBps": round(step_bytes / (hip_kernels_us * 1e-6) / 1e12, 3),
        "round_ms": round(round_ms, 4),
        "rounds": a.rounds, "rounds_forward_ms": round(float(np.median(fw)), 4),
        "backward_ms": round(float(np.median(bw)), 4),
        "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
