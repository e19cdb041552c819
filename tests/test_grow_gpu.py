"""-m gpu: the growth step (gi_grow_graphs) and the sync-free generation loop (graphinvent_amd.generator).

1. The step against the torch bookkeeping of oracle/callers_oracle.GeneratorOracle (the reference's
   copy_terminated_graphs / apply_actions / reset_graphs, restated) fed the same draw: bit-identical state every round.
2. build_graphs with the stub model reproduces tests/golden/golden_grow.npz (the unmodified reference loop).
3. build_graphs with the drop-in GGNN reproduces golden_generator.npz in the blocking, sync-free and captured modes, for
   several poll intervals.
4. No read-back between polls.
5. Rounds enqueued after the target (or an error) change nothing; indices the reference rejects write nothing."""
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

from graphinvent_amd import lib as L
from graphinvent_amd import ops
from graphinvent_amd.generator import build_graphs, grow_step, new_state
from graphinvent_amd.sampler import _unravel, sample_actions_raw
from oracle import callers_oracle as CO
from oracle import ggnn_oracle as O
from tests import grow_oracle as GO
from tests.golden import ref_callers as RC

pytestmark = pytest.mark.gpu
DEV = "cuda"
STATE = ("nodes", "edges", "n_nodes", "likelihoods", "generated_nodes", "generated_edges", "generated_n_nodes",
         "generated_likelihoods", "properly_terminated")


def gen_constants(N, groups, Fe, chirality=False, imp_h=False):
    """The constants fields GeneratorOracle reads (parameters/constants.py)."""
    n_imp = groups[2] if imp_h else 0
    d = dict(device=DEV, max_n_nodes=N, n_atom_types=groups[0], n_formal_charge=groups[1], n_imp_H=n_imp,
             n_chirality=groups[-1] if chirality else 0, use_explicit_H=False, ignore_H=not imp_h,
             use_chirality=chirality, dim_nodes=[N, sum(groups)], dim_edges=[N, N, Fe],
             dim_f_add=[N, *groups, Fe], dim_f_conn=[N, Fe])
    return namedtuple("CONSTANTS", sorted(d))(**d)


def snapshot(obj):
    return {k: getattr(obj, k).clone() for k in STATE}


# ---- 1 ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,N", [(64, 5), (64, 13), (1000, 5), (1000, 13)])
def test_step_equals_the_torch_bookkeeping_bit_for_bit(B, N):
    groups, Fe, rounds, Lc = [5, 3], 3, 40, 48
    c = gen_constants(N, groups, Fe)
    ref = CO.GeneratorOracle(None, B, c, None)
    C = (rounds + 1) * B                     # room for every round's finished graphs: torch never indexes past a buffer
    ref.likelihoods = torch.zeros(B, Lc, device=DEV)
    ref.generated_nodes = torch.zeros(C, *c.dim_nodes, device=DEV)
    ref.generated_edges = torch.zeros(C, *c.dim_edges, device=DEV)
    ref.generated_n_nodes = torch.zeros(C, dtype=torch.int8, device=DEV)
    ref.generated_likelihoods = torch.zeros(C, Lc, device=DEV)
    ref.properly_terminated = torch.zeros(C, dtype=torch.int8, device=DEV)
    dut = snapshot(ref)
    state = new_state(B, C, DEV)
    sub, A = [*groups, Fe], int(np.prod(groups)) * Fe
    W = N * A + N * Fe + 1
    g = torch.Generator(device=DEV).manual_seed(1000 * N + B)
    n, seen = 0, np.zeros(4, int)
    for r in range(rounds):
        # adversarial logits: flat noise plus a per-round push towards terminate, connect or add-to-node-0
        logits = torch.randn(B, W, device=DEV, generator=g) * 2.0
        logits[:, -1] += float(r % 3 == 0) * 3.0
        logits[:, N * A:N * A + N * Fe] += float(r % 4 == 1) * 3.0
        logits[:, :A] += float(r % 5 == 2) * 4.0
        u = torch.rand(B, device=DEV, generator=g)
        action, like, flags = sample_actions_raw(logits, ref.n_nodes, ref.edges, A, uniform=u)
        add, conn, term, invalid = _unravel(action, flags, sub)
        ref.properly_terminated[n:(n + len(term))] = 1                              # GraphGenerator.py:127-157
        idc = torch.cat((term, invalid))
        idc = idc[idc != 0]
        n = ref.copy_terminated_graphs(idc, n, r, like)
        ref.apply_actions(add, conn, r, like)
        ref.reset_graphs(idc)
        grow_step(*(dut[k] for k in STATE), action, like, flags, c.dim_f_add, c.dim_f_conn, state)
        for k in STATE:
            assert torch.equal(dut[k], getattr(ref, k)), (r, k)
        st = state[:4].tolist()
        assert st == [n, r + 1, C, 0], (r, st, n)
        kind = action[:, 0].cpu().numpy()
        seen += [np.sum(kind == 0), np.sum(kind == 1), np.sum(kind == 2), int((flags & 1).sum())]
    assert (seen > 0).all() and n > B, (seen, n)


# ---- 2 ------------------------------------------------------------------------------------------------------------

class _Gen:
    """The reference generator's fields after __init__ (GraphGenerator.py:27-43), on the device."""

    def __init__(self, model, B, N, Fn, Fe, Lc=None, C=None):
        s = GO.new_state(B, N, Fn, Fe, Lc or 2 * N, C or 2 * B)
        self.model, self.batch_size = model, B
        for k in STATE:
            setattr(self, k, torch.from_numpy(s[k]).to(DEV))


@pytest.mark.parametrize("name", ["atoms_charges", "imp_h_chirality", "index_error"])
def test_build_graphs_reproduces_the_stub_golden(golden_dir, name):
    G = np.load(os.path.join(golden_dir, "golden_grow.npz"))
    p = f"{name}::cfg::"
    cfg = {k[len(p):]: G[k].tolist() for k in G.files if k.startswith(p)}
    N, groups, Fe, dim_f_add, dim_f_conn = GO.config_dims(cfg)
    B = int(cfg["B"])
    gen = _Gen(GO.StubModel(cfg), B, N, sum(groups), Fe)
    u = torch.from_numpy(CO.InverseCdfDraws(int(cfg["draw_seed"]), B).u[:64].astype(np.float32))
    raised = int(G[f"{name}::raised_round"])
    if raised >= 0:
        with pytest.raises(IndexError):
            build_graphs(gen, dim_f_add, dim_f_conn, uniforms=u, poll_every=3)
        assert gen.generation_rounds == raised
        return
    n = build_graphs(gen, dim_f_add, dim_f_conn, uniforms=u, poll_every=3)
    assert (n, gen.generation_rounds) == (int(G[f"{name}::n_generated"]), int(G[f"{name}::rounds"]))
    for k in STATE:
        got, want = getattr(gen, k).cpu().numpy(), G[f"{name}::{k}"]
        if "likelihoods" in k:
            assert np.all(np.abs(got - want) <= 1e-5 * np.abs(want)), k     # the kernel's fp32 softmax, not torch's
            assert np.array_equal(got == 0, want == 0), k
        else:
            assert np.array_equal(got.astype(want.dtype), want), k


# ---- 3 and 4 ------------------------------------------------------------------------------------------------------

def _ggnn_generator(golden_dir):
    from graphinvent_amd.gnn import mpnn
    G = np.load(os.path.join(golden_dir, "golden_generator.npz"))
    cfg = O.make_config(**{str(k): int(v) for k, v in zip(G["cfg_keys"], G["cfg_vals"])})
    consts = RC.as_constants(RC.constants_dict("cuda", cfg, "/nonexistent", batch_size=100, epochs=1))
    model = mpnn.GGNN(constants=consts)
    model.load_state_dict({k[3:]: torch.from_numpy(G[k]) for k in G.files if k.startswith("w::")})
    model = model.to(DEV).eval()
    u = torch.from_numpy(CO.InverseCdfDraws(int(G["draw_seed"]), int(G["batch"])).u[:64].astype(np.float32))
    return G, consts, model, u


def _sync_debug_honoured() -> bool:
    torch.cuda.set_sync_debug_mode("error")
    try:
        torch.ones(1, device=DEV).item()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode(0)


@pytest.mark.parametrize("mode", ["blocking", "sync_free", "capture"])
def test_build_graphs_with_the_ggnn_builds_the_reference_graphs(golden_dir, mode):
    G, consts, model, u = _ggnn_generator(golden_dir)
    model.sync_free = mode == "sync_free"
    strict = mode != "blocking" and _sync_debug_honoured()
    print(f"\n[{mode}] torch.cuda.set_sync_debug_mode honoured on this build: {_sync_debug_honoured()}")
    results = []
    for poll in (1, 5, 64):
        gen = CO.GeneratorOracle(model, int(G["batch"]), consts, None)
        rb0 = dict(ops.READBACKS)
        # The torch of the ROCm build this was written on honours set_sync_debug_mode: there the rounds run under
        # "error", and any host synchronisation outside the loop's own polls raises. Where it is not honoured, the
        # test relies on ops.READBACKS alone.
        if strict:
            torch.cuda.set_sync_debug_mode("error")
        try:
            n = build_graphs(gen, consts.dim_f_add, consts.dim_f_conn, uniforms=u, poll_every=poll,
                             capture=mode == "capture")
        finally:
            torch.cuda.set_sync_debug_mode(0)
        if mode != "blocking":               # 4: no read-back in any round
            assert ops.READBACKS["blocking"] == rb0["blocking"] and ops.READBACKS["prefetched"] == rb0["prefetched"]
        assert model.sync_free == (mode == "sync_free")                  # restored
        assert (n, gen.generation_rounds) == (int(G["n_generated"]), int(G["rounds"])), (mode, poll)
        assert np.array_equal(gen.generated_n_nodes.cpu().numpy(), G["n_nodes"])
        assert np.array_equal(gen.generated_nodes.cpu().numpy().astype(np.int8), G["nodes"])
        assert np.array_equal(gen.generated_edges.cpu().numpy().astype(np.int8), G["edges"])
        assert np.array_equal(gen.properly_terminated.cpu().numpy(), G["terminated"])
        like, ref = gen.generated_likelihoods.cpu().numpy(), G["likelihoods"]
        assert np.abs(like - ref).max() < 1e-4 * ref.max()
        results.append(snapshot(gen))
    for other in results[1:]:                # the poll interval changes nothing, bit for bit
        for k in STATE:
            assert torch.equal(other[k], results[0][k]), (mode, k)


# ---- 5 ------------------------------------------------------------------------------------------------------------

def _frozen_rounds_change_nothing(gen, c, state, B, A, W, k=10):
    before, st0 = snapshot(gen), state.clone()
    g = torch.Generator(device=DEV).manual_seed(7)
    for _ in range(k):
        logits = torch.randn(B, W, device=DEV, generator=g) * 3
        grow_step(*(getattr(gen, n) for n in STATE), *sample_actions_raw(logits, gen.n_nodes, gen.edges, A),
                  c.dim_f_add, c.dim_f_conn, state)
    torch.cuda.synchronize()
    for n in STATE:
        assert torch.equal(getattr(gen, n), before[n]), n
    assert torch.equal(state[:4], st0[:4])


def test_rounds_after_the_target_or_an_error_change_nothing():
    B, N, groups, Fe = 64, 6, [5, 3], 3
    c = gen_constants(N, groups, Fe)
    A = int(np.prod(groups)) * Fe
    W = N * A + N * Fe + 1
    gen = _Gen(None, B, N, sum(groups), Fe)
    state = new_state(B, B, DEV)
    g = torch.Generator(device=DEV).manual_seed(3)
    for r in range(2 * N):
        logits = torch.randn(B, W, device=DEV, generator=g) * 2
        logits[:, -1] += 2
        grow_step(*(getattr(gen, n) for n in STATE), *sample_actions_raw(logits, gen.n_nodes, gen.edges, A),
                  c.dim_f_add, c.dim_f_conn, state)
        if int(state[0]) >= B:
            break
    assert int(state[0]) >= B and int(state[3]) == 0
    _frozen_rounds_change_nothing(gen, c, state, B, A, W)

    # r >= L: the round writes nothing and reports IndexError's bit; later rounds are frozen
    gen = _Gen(None, B, N, sum(groups), Fe, Lc=4)
    state = new_state(B, B, DEV)
    state[1] = 4
    before = snapshot(gen)
    logits = torch.randn(B, W, device=DEV, generator=g) * 2
    logits[:, -1] += 3                                    # with terminations, so that the round would copy and reset
    grow_step(*(getattr(gen, n) for n in STATE), *sample_actions_raw(logits, gen.n_nodes, gen.edges, A),
              c.dim_f_add, c.dim_f_conn, state)
    assert state[:4].tolist() == [0, 4, B, L.GROW_ERR_ROUND]
    for n in STATE:
        assert torch.equal(getattr(gen, n), before[n]), n
    _frozen_rounds_change_nothing(gen, c, state, B, A, W)

    # more finished graphs than generated rows, and an action index out of range
    gen = _Gen(None, B, N, sum(groups), Fe, C=2)
    state = new_state(B, B, DEV)
    action, like, flags = sample_actions_raw(logits, gen.n_nodes, gen.edges, A)
    before = snapshot(gen)
    grow_step(*(getattr(gen, n) for n in STATE), action, like, flags, c.dim_f_add, c.dim_f_conn, state)
    assert state[:4].tolist() == [0, 0, B, L.GROW_ERR_CAPACITY]
    gen = _Gen(None, B, N, sum(groups), Fe)
    state = new_state(B, B, DEV)
    before = snapshot(gen)
    bad = action.clone()
    bad[5] = torch.tensor([0, N, 0, 1], dtype=torch.int32)          # node_to == N
    grow_step(*(getattr(gen, n) for n in STATE), bad, like, flags, c.dim_f_add, c.dim_f_conn, state)
    assert state[:4].tolist() == [0, 0, B, L.GROW_ERR_ACTION]
    for n in STATE:
        assert torch.equal(getattr(gen, n), before[n]), n
