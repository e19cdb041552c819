"""-m gpu: seeded generation (gi_grow_seed_init, gi_grow_graphs_seeded, gi_grow_graphs_rl_seeded; SeedBank and the
``seeds=`` argument of graphinvent_amd.generator) and the likelihood of a completion (``given_actions``).

1. The first fill and the step against the numpy model of tests/seed_grow_model.py, bit for bit on every state tensor,
   the slots' seeds and ``gen_seed``, at odd seed offsets and for banks smaller and larger than the batch.
2. The whole loop with grow_oracle's stub logits and pinned uniforms equals the CPU model in the blocking, sync-free
   and captured modes, with no host synchronisation inside the loop.
3. A bank of the empty seed alone reproduces golden_grow.npz (the unmodified reference) through the seeded entry points.
4. With the tiny golden GGNN every generated row contains its seed.
5. Rounds enqueued after the target or an error change nothing, the slots' seeds included.
6. RL: build_graphs_rl(seeds=...) against the restated loop of tests/rl_callers.py with a seeded
   initialize_graph_batch / reset_graphs: graphs, both likelihood streams, provenance, both models' gradients.
7. given_actions on the device against the CPU test's values, its gradient, and the values it refuses.
8. SeedBank's refusals, each naming the rule."""
import os

import numpy as np
import pytest
import torch

from graphinvent_amd import lib as L
from graphinvent_amd import likelihood as LL
from graphinvent_amd import ops, routes, sampler
from graphinvent_amd.generator import (SeedBank, build_graphs, build_graphs_rl, grow_step, new_state, seed_init)
from graphinvent_amd.gnn import mpnn
from graphinvent_amd.sampler import sample_actions_raw
from oracle import callers_oracle as CO
from oracle import ggnn_oracle as O
from tests import grow_oracle as GO
from tests import rl_callers as RL
from tests import seed_grow_model as SM
from tests.test_grow_gpu import STATE, _Gen, _ggnn_generator, _sync_debug_honoured, snapshot
from tests.test_grow_rl_gpu import gen_constants as rl_constants
from tests.test_likelihood_cpu import golden, oracle_logits, route_set
from tests.test_seeded_cpu import completion_cases

pytestmark = pytest.mark.gpu
DEV = "cuda"
_CACHE = {}


def _dev(x, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dtype)


def device_bank(bank, dim_f_add, dim_f_conn, **kw):
    return SeedBank(_dev(bank["nodes"]), _dev(bank["edges"]), dim_f_add, dim_f_conn, **kw)


def slot_seeds(state, B):
    return state[L.GROW_STATE_WORDS + 2 * B:L.GROW_STATE_WORDS + 3 * B]


# ---- 1 ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [1, 3, 100])
@pytest.mark.parametrize("B,N,groups", [(64, 5, [4, 3]), (64, 13, [5, 3])])
def test_first_fill_and_step_equal_the_numpy_model_bit_for_bit(B, N, groups, S):
    Fe, rounds = 3, 12
    Fn, Lc, C = sum(groups), rounds + 2, (rounds + 1) * B
    if N == 5:
        assert (N * Fn, N * N * Fe) == (35, 75)            # seed 1 starts at an odd byte of both arrays
    dim_f_add, dim_f_conn = [N, *groups, Fe], [N, Fe]
    bank = SM.mixed_bank(N, groups, Fe, S, seed=B + N)
    dbank = device_bank(bank, dim_f_add, dim_f_conn)
    assert len(dbank) == S and np.array_equal(dbank.n_nodes.cpu().numpy(), bank["n_nodes"])
    n_edges = bank["edges"].reshape(S, -1).sum(1) // 2
    assert np.array_equal(dbank.n_actions.cpu().numpy(), np.where(bank["n_nodes"] == 0, 0, n_edges + 1))
    s = SM.new_seeded_state(B, N, Fn, Fe, Lc, C, bank)
    s["target"] = C
    fresh = GO.new_state(B, N, Fn, Fe, Lc, C)
    dut = {k: _dev(fresh[k]) for k in STATE}
    dut["likelihoods"][1:] = 7.0                         # the first fill zeroes the likelihood rows, not row 0's
    state = new_state(B, C, DEV, seeded=True)
    gen_seed = torch.full((C,), -1, dtype=torch.int32, device=DEV)
    seed_init(dut["nodes"], dut["edges"], dut["n_nodes"], dut["likelihoods"], state, dbank)
    for k in STATE:
        assert np.array_equal(dut[k].cpu().numpy(), s[k]), ("init", k)
    assert np.array_equal(slot_seeds(state, B).cpu().numpy(), s["slot_seed"])
    A = int(np.prod(groups)) * Fe
    W = N * A + N * Fe + 1
    g = torch.Generator(device=DEV).manual_seed(1000 * N + B + S)
    seen = np.zeros(4, int)
    for r in range(rounds):
        logits = torch.randn(B, W, device=DEV, generator=g) * 2.0
        logits[:, -1] += float(r % 3 == 0) * 3.0
        logits[:, N * A:N * A + N * Fe] += float(r % 4 == 1) * 3.0
        logits[:, :A] += float(r % 5 == 2) * 4.0
        u = torch.rand(B, device=DEV, generator=g)
        action, like, flags = sample_actions_raw(logits, dut["n_nodes"], dut["edges"], A, uniform=u)
        grow_step(*(dut[k] for k in STATE), action, like, flags, dim_f_add, dim_f_conn, state, seeds=dbank,
                  generated_seed=gen_seed)
        a, f = action.cpu().numpy(), flags.cpu().numpy()
        SM.seeded_round(s, a, like.cpu().numpy(), f, groups, Fe, bank)
        assert s["error"] == 0
        for k in STATE:
            assert np.array_equal(dut[k].cpu().numpy(), s[k]), (r, k)
        assert np.array_equal(gen_seed.cpu().numpy(), s["gen_seed"]), r
        assert np.array_equal(slot_seeds(state, B).cpu().numpy(), s["slot_seed"]), r
        assert state[:4].tolist() == [s["n"], r + 1, C, 0]
        seen += [np.sum(a[:, 0] == 0), np.sum(a[:, 0] == 1), np.sum(a[:, 0] == 2), int((f & 1).sum())]
    assert (seen > 0).all() and s["n"] > B, (seen, s["n"])
    if S == 3:
        assert set(s["gen_seed"][:s["n"]].tolist()) == {0, 1, 2}


# ---- 2 ------------------------------------------------------------------------------------------------------------

def _config(golden_dir, name):
    G = np.load(os.path.join(golden_dir, "golden_grow.npz"))
    p = f"{name}::cfg::"
    return G, {k[len(p):]: G[k].tolist() for k in G.files if k.startswith(p)}


class DeviceStub(torch.nn.Module):
    """grow_oracle's stub logits of rounds 0 .. R - 1, uploaded once; the round counter lives on the device, so a
    forward is a gather and an increment: no host synchronisation, and capturable.  Under ``capture`` the calls made
    outside a stream capture (the loop's warm-up, which applies no round) return round 0 and do not count."""

    def __init__(self, cfg, rounds, capture=False):
        super().__init__()
        self.z = torch.from_numpy(np.stack([GO.stub_logits(cfg, r) for r in range(rounds)])).to(DEV)
        self.k = torch.zeros(1, dtype=torch.long, device=DEV)
        self.capture = capture

    def forward(self, nodes, edges):
        if self.capture and not torch.cuda.is_current_stream_capturing():
            return self.z[0].clone()
        out = self.z[self.k.clamp(max=self.z.shape[0] - 1)][0]      # (rounds enqueued past the last one: frozen anyway)
        self.k += 1
        return out


def _loop_reference(golden_dir, name, S):
    key = ("loop", name, S)
    if key not in _CACHE:
        _, cfg = _config(golden_dir, name)
        N, groups, Fe, _, _ = GO.config_dims(cfg)
        bank = SM.mixed_bank(N, groups, Fe, S)
        s, draw = SM.run_seeded_oracle(cfg, bank)
        assert s["error"] == 0 and draw.margin > 1e-4
        _CACHE[key] = (cfg, bank, s)
    return _CACHE[key]


@pytest.mark.parametrize("mode", ["blocking", "sync_free", "capture"])
@pytest.mark.parametrize("name,S", [("atoms_charges", 3), ("atoms_charges", 100), ("imp_h_chirality", 1)])
def test_seeded_loop_equals_the_cpu_model_in_every_mode(golden_dir, name, S, mode):
    cfg, bank, ref = _loop_reference(golden_dir, name, S)
    N, groups, Fe, dim_f_add, dim_f_conn = GO.config_dims(cfg)
    B = int(cfg["B"])
    dbank = device_bank(bank, dim_f_add, dim_f_conn)
    u = torch.from_numpy(CO.InverseCdfDraws(int(cfg["draw_seed"]), B).u[:64].astype(np.float32)).to(DEV)
    assert ref["round"] <= 2 * N
    model = DeviceStub(cfg, 64, capture=mode == "capture")
    if mode == "sync_free":
        model.sync_free = True
    gen = _Gen(model, B, N, sum(groups), Fe)
    torch.cuda.synchronize()
    strict = mode != "blocking" and _sync_debug_honoured()
    rb0 = dict(ops.READBACKS)
    if strict:                               # any host synchronisation outside the loop's own polls raises
        torch.cuda.set_sync_debug_mode("error")
    try:
        n = build_graphs(gen, dim_f_add, dim_f_conn, uniforms=u, poll_every=3, capture=mode == "capture",
                         seeds=dbank)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert ops.READBACKS["blocking"] == rb0["blocking"] and ops.READBACKS["prefetched"] == rb0["prefetched"]
    assert (n, gen.generation_rounds) == (ref["n"], ref["round"])
    for k in STATE:
        got, want = getattr(gen, k).cpu().numpy(), ref[k]
        if "likelihoods" in k:                                   # the kernel's fp32 softmax, not torch's
            assert np.all(np.abs(got - want) <= 1e-5 * np.abs(want)), k
            assert np.array_equal(got == 0, want == 0), k
        else:
            assert np.array_equal(got, want), k
    assert gen.generated_seed.dtype == torch.int32 and gen.generated_seed.is_cuda
    assert np.array_equal(gen.generated_seed.cpu().numpy(), ref["gen_seed"])


# ---- 3 ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["atoms_charges", "imp_h_chirality", "index_error"])
def test_empty_seed_bank_reproduces_the_stub_golden(golden_dir, name):
    G, cfg = _config(golden_dir, name)
    N, groups, Fe, dim_f_add, dim_f_conn = GO.config_dims(cfg)
    B = int(cfg["B"])
    bank = device_bank(SM.empty_bank(N, sum(groups), Fe, 2), dim_f_add, dim_f_conn)
    assert bank.n_nodes.tolist() == [0, 0] and bank.n_actions.tolist() == [0, 0]
    gen = _Gen(GO.StubModel(cfg), B, N, sum(groups), Fe)
    u = torch.from_numpy(CO.InverseCdfDraws(int(cfg["draw_seed"]), B).u[:64].astype(np.float32))
    raised = int(G[f"{name}::raised_round"])
    if raised >= 0:
        with pytest.raises(IndexError):
            build_graphs(gen, dim_f_add, dim_f_conn, uniforms=u, poll_every=3, seeds=bank)
        assert gen.generation_rounds == raised
        return
    n = build_graphs(gen, dim_f_add, dim_f_conn, uniforms=u, poll_every=3, seeds=bank)
    assert (n, gen.generation_rounds) == (int(G[f"{name}::n_generated"]), int(G[f"{name}::rounds"]))
    for k in STATE:
        got, want = getattr(gen, k).cpu().numpy(), G[f"{name}::{k}"]
        if "likelihoods" in k:
            assert np.all(np.abs(got - want) <= 1e-5 * np.abs(want)), k     # the kernel's fp32 softmax, not torch's
            assert np.array_equal(got == 0, want == 0), k
        else:
            assert np.array_equal(got.astype(want.dtype), want), k
    seeds = gen.generated_seed.cpu().numpy()
    assert ((seeds[:n] >= 0) & (seeds[:n] < 2)).all() and (seeds[n:] == -1).all()


# ---- 4 ------------------------------------------------------------------------------------------------------------

def test_with_the_golden_ggnn_every_generated_row_contains_its_seed(golden_dir):
    G, consts, model, u = _ggnn_generator(golden_dir)
    B = int(G["batch"])
    N, Fe = consts.dim_f_add[0], consts.dim_f_add[-1]
    groups = list(consts.dim_f_add[1:-1])
    S = 5
    bank = SM.mixed_bank(N, groups, Fe, S, seed=4)
    dbank = device_bank(bank, consts.dim_f_add, consts.dim_f_conn)
    gen = CO.GeneratorOracle(model, B, consts, None)
    n = build_graphs(gen, consts.dim_f_add, consts.dim_f_conn, uniforms=u.to(DEV), seeds=dbank)
    assert n >= B
    seed = gen.generated_seed[:n].long()
    assert int(seed.min()) >= 0 and int(seed.max()) < S and bool((gen.generated_seed[n:] == -1).all())
    # round-robin: over the first fill and the refills, seeds are handed out in bank order; a row's seed is one handed
    # out before the row was written, and every seed of the bank is used
    handed = torch.cat((torch.arange(B - 1, device=DEV), B - 1 + torch.arange(n, device=DEV))) % S
    assert set(seed.tolist()) == set(range(S))
    counts = torch.bincount(seed, minlength=S)
    assert bool((counts <= torch.bincount(handed, minlength=S)).all())
    sn, se = dbank.nodes[seed].float(), dbank.edges[seed].float()
    ns = dbank.n_nodes[seed].long()
    gn, ge = gen.generated_nodes[:n], gen.generated_edges[:n]
    idx = torch.arange(N, device=DEV)
    inside = idx[None, :] < ns[:, None]                                      # [n, N]: the seed's nodes
    assert torch.equal(gn * inside[:, :, None], sn)                          # the first n_s node rows are the seed's
    assert bool((gen.generated_n_nodes[:n].long() >= ns).all())
    pair = (inside[:, :, None] & inside[:, None, :])[..., None]              # [n, N, N, 1]
    assert bool(((ge * pair) >= se).all())                                   # a superset of the seed's edges
    extra = ((ge * pair) != 0) & (se == 0)
    last = (idx[None, :] == (ns - 1)[:, None])
    touches = (last[:, :, None] | last[:, None, :])[..., None]
    assert bool((~extra | touches).all())                                    # every extra edge touches node n_s - 1
    # the likelihood row holds the completion alone: one contiguous run of columns, as long as the actions after the
    # (re)start — one per bond added, the first atom of an empty seed, and the terminate (or the refused action)
    like = gen.generated_likelihoods[:n]
    nz = like != 0
    cols = torch.arange(like.shape[1], device=DEV)
    lo = torch.where(nz, cols, like.shape[1]).min(1).values
    hi = torch.where(nz, cols, -1).max(1).values
    assert bool((nz.sum(1) == hi - lo + 1).all())
    bonds = lambda e: (e != 0).flatten(1).sum(1) // 2
    first_atom = ((ns == 0) & (gen.generated_n_nodes[:n] > 0)).long()
    assert torch.equal(nz.sum(1), bonds(ge) - bonds(se) + first_atom + 1)
    assert int(ns.max()) == N and int(ns.min()) == 0                         # a full and an empty seed were grown
    assert bool(((gen.generated_n_nodes[:n].long() > ns)).any())


# ---- 5 ------------------------------------------------------------------------------------------------------------

def _frozen(gen, dim_f_add, dim_f_conn, state, dbank, gen_seed, B, A, W, k=6):
    before, st0, gs0 = snapshot(gen), state.clone(), gen_seed.clone()
    g = torch.Generator(device=DEV).manual_seed(7)
    for _ in range(k):
        logits = torch.randn(B, W, device=DEV, generator=g) * 3
        grow_step(*(getattr(gen, n) for n in STATE), *sample_actions_raw(logits, gen.n_nodes, gen.edges, A),
                  dim_f_add, dim_f_conn, state, seeds=dbank, generated_seed=gen_seed)
    torch.cuda.synchronize()
    for n in STATE:
        assert torch.equal(getattr(gen, n), before[n]), n
    assert torch.equal(state[:4], st0[:4]) and torch.equal(slot_seeds(state, B), slot_seeds(st0, B))
    assert torch.equal(gen_seed, gs0)


def test_rounds_after_the_target_or_an_error_change_nothing_seeds_included():
    B, N, groups, Fe = 64, 5, [4, 3], 3
    dim_f_add, dim_f_conn = [N, *groups, Fe], [N, Fe]
    A = int(np.prod(groups)) * Fe
    W = N * A + N * Fe + 1
    dbank = device_bank(SM.mixed_bank(N, groups, Fe, 3), dim_f_add, dim_f_conn)

    def fresh(Lc=None):
        gen = _Gen(None, B, N, sum(groups), Fe, Lc=Lc)
        state = new_state(B, B, DEV, seeded=True)
        gen_seed = torch.full((2 * B,), -1, dtype=torch.int32, device=DEV)
        seed_init(gen.nodes, gen.edges, gen.n_nodes, gen.likelihoods, state, dbank)
        return gen, state, gen_seed

    gen, state, gen_seed = fresh()
    g = torch.Generator(device=DEV).manual_seed(3)
    for r in range(2 * N):
        logits = torch.randn(B, W, device=DEV, generator=g) * 2
        logits[:, -1] += 2
        grow_step(*(getattr(gen, n) for n in STATE), *sample_actions_raw(logits, gen.n_nodes, gen.edges, A),
                  dim_f_add, dim_f_conn, state, seeds=dbank, generated_seed=gen_seed)
        if int(state[0]) >= B:
            break
    assert int(state[0]) >= B and int(state[3]) == 0
    _frozen(gen, dim_f_add, dim_f_conn, state, dbank, gen_seed, B, A, W)

    # r >= L (the reference's IndexError): the round writes nothing and reports the bit; later rounds are frozen
    gen, state, gen_seed = fresh(Lc=4)
    state[1] = 4
    before, seeds0 = snapshot(gen), slot_seeds(state, B).clone()
    logits = torch.randn(B, W, device=DEV, generator=g) * 2
    logits[:, -1] += 3                                    # with terminations, so that the round would copy and refill
    grow_step(*(getattr(gen, n) for n in STATE), *sample_actions_raw(logits, gen.n_nodes, gen.edges, A),
              dim_f_add, dim_f_conn, state, seeds=dbank, generated_seed=gen_seed)
    assert state[:4].tolist() == [0, 4, B, L.GROW_ERR_ROUND]
    for n in STATE:
        assert torch.equal(getattr(gen, n), before[n]), n
    assert torch.equal(slot_seeds(state, B), seeds0) and bool((gen_seed == -1).all())
    _frozen(gen, dim_f_add, dim_f_conn, state, dbank, gen_seed, B, A, W)


# ---- 6 ------------------------------------------------------------------------------------------------------------

class SeededRLOracle(RL.GeneratorRLOracle):
    """The restated RL loop with a seed bank: ``initialize_graph_batch`` fills slot g >= 1 from seed (g - 1) mod S,
    ``reset_graphs`` refills the graph written to generated row ``row`` from seed (B - 1 + row) mod S."""

    def __init__(self, agent, prior, batch_size, constants, bank, sampler=None):
        self.bank = {k: _dev(v) for k, v in bank.items()}
        self.S = len(bank["n_nodes"])
        super().__init__(agent, prior, batch_size, constants, sampler=sampler)
        self.generated_seed = torch.full((2 * batch_size,), -1, dtype=torch.int32, device=DEV)

    def _fill(self, slots, seeds):
        self.nodes[slots] = self.bank["nodes"][seeds].float()
        self.edges[slots] = self.bank["edges"][seeds].float()
        self.n_nodes[slots] = self.bank["n_nodes"][seeds]
        self.slot_seed[slots] = seeds.to(torch.int32)

    def initialize_graph_batch(self):
        super().initialize_graph_batch()
        B = self.batch_size
        self.slot_seed = torch.full((B,), -1, dtype=torch.int32, device=DEV)
        slots = torch.arange(1, B, device=DEV)
        self._fill(slots, (slots - 1) % self.S)

    def copy_terminated_graphs(self, terminate_idc, n_graphs_generated, generation_round, agent_like, prior_like):
        self._row0 = n_graphs_generated
        return super().copy_terminated_graphs(terminate_idc, n_graphs_generated, generation_round, agent_like,
                                              prior_like)

    def reset_graphs(self, idc):
        super().reset_graphs(idc)
        if len(idc) > 0:
            idc = idc.long()
            rows = self._row0 + torch.arange(len(idc), device=DEV)
            self.generated_seed[rows] = self.slot_seed[idc]
            self._fill(idc, (self.batch_size - 1 + rows) % self.S)


def _rl_models(N, atoms, charges, seed=11):
    cfg = O.shaped_config(atoms, charges, N)
    P = O.init_params(cfg, seed=seed, model="GGNN")
    agent = mpnn.GGNN(O.as_constants(dict(cfg, device=DEV)))
    agent.load_state_dict(P)
    prior = RL.perturbed_prior(agent, seed=seed + 1)
    return agent.to(DEV).eval(), prior.to(DEV).eval()


def test_build_graphs_rl_with_seeds_equals_the_restated_seeded_loop():
    B, N, groups, Fe, S = 64, 5, [4, 3], 3, 3
    c = rl_constants(N, groups, Fe)
    agent, prior = _rl_models(N, *groups)
    bank = SM.mixed_bank(N, groups, Fe, S, seed=6)
    dbank = device_bank(bank, c.dim_f_add, c.dim_f_conn)
    u = torch.rand(64, B, generator=torch.Generator().manual_seed(3))
    scores = torch.rand(B, generator=torch.Generator().manual_seed(4)).to(DEV)
    uniq = torch.ones(B, device=DEV)

    class Draws:
        round = 0

        def __call__(self, agent_logits, prior_logits, n_nodes, edges):
            self.round += 1
            return sampler.sample_actions_rl(agent_logits, prior_logits, n_nodes, edges, c.dim_f_add, c.dim_f_conn,
                                             uniform=u[self.round - 1].to(DEV))

    keys = ("generated_nodes", "generated_edges", "generated_n_nodes", "properly_terminated",
            "generated_agent_likelihoods", "generated_prior_likelihoods", "nodes", "edges", "n_nodes",
            "agent_likelihoods", "prior_likelihoods", "generated_seed")
    results = []
    for restated in (True, False):
        for m in (agent, prior):
            for p in m.parameters():
                p.grad = None
        if restated:
            gen = SeededRLOracle(agent, prior, B, c, bank, sampler=Draws())
            n, rounds = gen.build_graphs(), gen.rounds
        else:
            gen = RL.GeneratorRLOracle(agent, prior, B, c)
            n = build_graphs_rl(gen, c.dim_f_add, c.dim_f_conn, uniforms=u, poll_every=2, seeds=dbank)
            rounds = gen.generation_rounds
        a_ll, p_ll = gen.loglikelihoods()
        loss = torch.mean(RL.compute_loss_component(scores, a_ll, p_ll, uniq, 0.5))
        loss.backward()
        grads = [p.grad.detach().clone() for m in (agent, prior) for p in m.parameters()]
        results.append((n, rounds, {k: getattr(gen, k).detach().clone() for k in keys}, grads))
    (n0, r0, s0, g0), (n1, r1, s1, g1) = results
    print(f"\nseeded RL, B = {B}: {n0} graphs in {r0} rounds")
    assert (n0, r0) == (n1, r1) and n0 >= B
    for k in keys:
        assert torch.equal(s0[k], s1[k]), k
    assert set(s1["generated_seed"][:n1].tolist()) == set(range(S))
    for i, (a, b) in enumerate(zip(g0, g1)):
        scale = float(a.abs().max())
        assert float((a - b).abs().max()) <= 1e-6 * max(scale, 1e-30), i


# ---- 7 ------------------------------------------------------------------------------------------------------------

def test_given_actions_on_the_device_against_the_cpu_values():
    from tests.test_likelihood_gpu import Recorder, _golden_model, _logit_slack, _molecules
    G = golden()
    _, _, hot, row_mol = route_set()[:4]
    dn, de, add, conn = _molecules()
    cases, row_step, lengths = completion_cases()
    model = _golden_model()
    with torch.no_grad():
        plain = LL.molecule_log_likelihood(model, dn, de, add, conn, batch_rows=256, by_kind=True)
        for name, (given, want, n_kept, keep) in cases.items():
            rec = Recorder(model)
            arg = _dev(given) if name != "between" else given.tolist()      # a device tensor or a sequence
            ll, kind = LL.molecule_log_likelihood(rec, dn, de, add, conn, batch_rows=256, by_kind=True,
                                                  given_actions=arg)
            slack, _ = _logit_slack(rec, oracle_logits())
            # test_likelihood_gpu.py's _assert_molecules_close bound, over the rows that stay
            bound = np.bincount(row_mol, weights=(1e-4 + 1e-4 * np.abs(G["row_ll"]) + 2 * slack) * keep, minlength=140)
            got = ll.cpu().numpy().astype(np.float64)
            err = np.abs(got - want)
            print(f"\n[{name}] max err {err.max():.2e}, max err / bound {(err / bound).max():.3f}")
            assert np.isfinite(got).all() and (err <= bound).all(), name
            assert torch.allclose(kind.sum(1), ll, rtol=1e-5, atol=1e-5)
            if name == "none":                                              # None is the same computation
                assert torch.equal(ll, plain[0]) and torch.equal(kind, plain[1])
            if name == "all":
                assert bool((kind[:, :2] == 0).all())
        for bad in (lengths.astype(np.int32), np.full(140, -1, np.int32)):
            with pytest.raises(ValueError, match="given_actions"):
                LL.molecule_log_likelihood(model, dn, de, add, conn, given_actions=_dev(bad))
        with pytest.raises(ValueError, match="given_actions"):
            LL.molecule_log_likelihood(model, dn, de, add, conn, given_actions=[0, 1])


def test_gradient_of_a_fully_given_molecule_is_the_terminate_rows_alone():
    from tests.test_likelihood_gpu import _golden_model, _molecules
    dn, de, add, conn = _molecules()
    _, _, lengths = completion_cases()
    M = 12
    W = int(np.prod(add)) + int(np.prod(conn)) + 1
    w = torch.linspace(0.5, 1.5, M, device=DEV)
    model = _golden_model()
    ll = LL.weighted_log_likelihood_backward(model, dn[:M], de[:M], add, conn, w, batch_rows=50,
                                             given_actions=_dev(lengths[:M] - 1, torch.int32))
    masked = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    model.zero_grad(set_to_none=True)
    # the terminate row of a route is the whole molecule with the last APD index hot
    rows = LL.row_log_likelihood(model(dn[:M], de[:M]), torch.full((M,), W - 1, dtype=torch.int32, device=DEV))
    (w * rows).sum().backward()
    assert torch.allclose(ll, rows.detach(), rtol=1e-5, atol=1e-5)
    for k, p in model.named_parameters():                     # test_likelihood_gpu.py's bar between two batchings
        scale = float(p.grad.abs().max())
        assert float((masked[k] - p.grad).abs().max()) <= 1e-3 * scale + 1e-7, k
    # and through autograd
    model.zero_grad(set_to_none=True)
    ll2 = LL.molecule_log_likelihood(model, dn[:M], de[:M], add, conn, batch_rows=50,
                                     given_actions=_dev(lengths[:M] - 1, torch.int32))
    (w * ll2).sum().backward()
    for k, p in model.named_parameters():
        scale = float(masked[k].abs().max())
        assert float((masked[k] - p.grad).abs().max()) <= 1e-3 * scale + 1e-7, k


# ---- 8 ------------------------------------------------------------------------------------------------------------

def _seed_molecules():
    """Three valid seeds of five atoms (N = 6, groups [4, 3], Fe = 3): a chain each."""
    N, groups, Fe = 6, [4, 3], 3
    nodes, edges = np.zeros((3, N, 7), np.int8), np.zeros((3, N, N, Fe), np.int8)
    for m in range(3):
        for i in range(5):
            nodes[m, i, (i + m) % 4] = 1
            nodes[m, i, 4 + i % 3] = 1
            if i:
                edges[m, i, i - 1, i % Fe] = edges[m, i - 1, i, i % Fe] = 1
    return nodes, edges, [N, *groups, Fe], [N, Fe]


@pytest.mark.parametrize("kind", ["disconnected", "later_node_only", "not_one_hot", "asymmetric"])
def test_seed_bank_refuses_invalid_seeds_naming_the_rule(kind):
    nodes, edges, add, conn = _seed_molecules()
    SeedBank(_dev(nodes), _dev(edges), add, conn)                            # valid as they are
    if kind == "disconnected":                                               # atoms {0, 1, 2} and {3, 4}
        edges[1, 3, 2] = edges[1, 2, 3] = 0
        bit = L.ROUTE_ERR_CONNECT
    elif kind == "later_node_only":                                          # node 1 bonded to node 2 alone
        edges[1, 1, 0] = edges[1, 0, 1] = 0
        edges[1, 2, 0, 1] = edges[1, 0, 2, 1] = 1
        bit = L.ROUTE_ERR_CONNECT
    elif kind == "not_one_hot":
        nodes[1, 2, :4] = 0
        nodes[1, 2, [0, 1]] = 1
        bit = L.ROUTE_ERR_ONEHOT
    else:
        edges[1, 3, 2] = 0
        bit = L.ROUTE_ERR_ASYMMETRIC
    with pytest.raises(ValueError) as e:
        SeedBank(_dev(nodes), _dev(edges), add, conn)
    assert routes.ERROR_MESSAGES[bit] in str(e.value) and "seed 1" in str(e.value)
    if kind == "later_node_only":                                            # a matter of node order: reorder mends it
        bank = SeedBank(_dev(nodes), _dev(edges), add, conn, reorder="bfs")
        assert bank.n_nodes.tolist() == [5, 5, 5] and bank.n_actions.tolist() == [5, 5, 5]
        assert int(routes.check(bank.nodes, bank.edges, add, conn).abs().sum()) == 0
    if kind == "disconnected":
        with pytest.raises(ValueError, match="not connected"):
            SeedBank(_dev(nodes), _dev(edges), add, conn, reorder="dfs")


def test_build_graphs_refuses_a_bank_of_other_dims():
    nodes, edges, add, conn = _seed_molecules()
    bank = SeedBank(_dev(nodes), _dev(edges), add, conn)
    for N, groups, Fe in ((5, [4, 3], 3), (6, [5, 3], 3), (6, [4, 3], 2)):
        gen = _Gen(None, 8, N, sum(groups), Fe)
        before = snapshot(gen)
        with pytest.raises(ValueError, match="N, Fn, Fe"):
            build_graphs(gen, [N, *groups, Fe], [N, Fe], seeds=bank)
        for k in STATE:
            assert torch.equal(getattr(gen, k), before[k]), k
    with pytest.raises(TypeError, match="SeedBank"):
        build_graphs(_Gen(None, 8, 6, 7, 3), add, conn, seeds=(nodes, edges))
