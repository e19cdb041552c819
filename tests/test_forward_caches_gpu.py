"""-m gpu: the inference caches of the fused models across call orders.

No-grad forwards keep two things across calls: the weights cache (``gi_graph.wcache``: the fp16x2 forward chain image,
its max |W| cells, the node-level layers' max |W| cells and the weights' range check) and the pass-0 row table
(``gi_graph.p0_cache``).  Once Python marks them valid they are trusted, so a derivation that is skipped or incomplete
shows up as wrong logits and nothing else.

Method: two models with identical weights see identical inputs, A with both caches on, B with both off (B derives
everything on every call).  After every forward of a scripted sequence A's logits equal B's bit for bit, and the last
forward of each sequence is checked against the fp64 oracle at the tolerance of the full-size parity tests.  Before its
first forward A's weights cache is filled with NaN, and so is the row area of its pass-0 table (header and hash words
stay zero: zero marks a free slot), so a pack that does not happen gives NaN or different logits rather than whatever
the allocator left in the buffer."""
import copy
import socket

import pytest
import torch

from graphinvent_amd import lib as L
from graphinvent_amd import synthetic
from graphinvent_amd.gnn import mpnn
from oracle import ggnn_oracle as O
from tests import mnn_oracle as MO

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4              # live graphs against the fp64 oracle (tests/test_model_gpu.py, tests/test_dims_gpu.py)
MASKED_TOL = 5e-3       # graphs without a bond: the energies' fl32(e - 1e6) quantisation (tests/test_attggnn_gpu.py)
ANCHOR_GRAPHS = 48      # graphs are independent: the oracle checks the first ones of the last batch
GDB13 = synthetic.SHAPES["gdb13"]
P0_ROWS_WORD = 8 + 33 * L.GI_MAX_GROUPS * 256   # PC_HDR + PC_DMAX + 4 PC_HCAP words (gi_compact.hip), GI_P0_MAX_CLASSES


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


# ---- set-up -------------------------------------------------------------------------------------------------------

class Pair:
    """Model A (both caches on, poisoned) and model B (both off) with identical weights."""

    def __init__(self, kind="GGNN", cfg=None, seed=3, sync_free=False, bounds=None):
        self.kind = kind
        if cfg is None:
            cfg = (MO.mnn_config if kind == "MNN" else O.shaped_config)(
                GDB13["n_atom_types"], GDB13["n_formal_charge"], GDB13["max_n_nodes"])
        self.cfg = cfg
        if kind == "MNN":
            self.P = MO.init_params(cfg, seed=seed)
            make = lambda: mpnn.MNN(MO.as_constants(dict(cfg, device="cuda")))
        else:
            self.P = O.init_params(cfg, seed=seed, model=kind)
            cls = mpnn.AttentionGGNN if kind == "AttGGNN" else mpnn.GGNN
            make = lambda: cls(O.as_constants(dict(cfg, device="cuda")))
        self.A, self.B = make(), make()
        for m, cache in ((self.A, True), (self.B, False)):
            m.load_state_dict(self.P)
            m.to(DEV).eval()
            m.cache_weights = cache
            m.cache_pass0 = cache and kind != "MNN"
            m.sync_free = sync_free
            m.sync_free_bounds = bounds
        self.n = 0
        poison(self.A)

    def forward(self, nodes, edges, tag=""):
        """One no-grad forward of each; A must equal B bit for bit."""
        with torch.no_grad():
            a = self.A(nodes, edges).clone()
            b = self.B(nodes, edges).clone()
        self.n += 1
        tag = f"forward {self.n} {tag}"
        assert torch.isfinite(b).all(), tag
        assert torch.equal(a, b), f"{tag}: cached != derived, max |d| {float((a - b).abs().nan_to_num(1e30).max())}"
        return b

    def sync_b(self):
        """B takes A's current weights (B has no cache: any write is fine)."""
        self.B.load_state_dict(self.A.state_dict())

    def anchor(self, nodes, edges, out):
        """The last forward against the fp64 oracle, on the first ANCHOR_GRAPHS graphs."""
        self.check_done()                       # (a sync-free forward past its bounds is reported, not computed)
        k = min(ANCHOR_GRAPHS, nodes.shape[0])
        n = nodes[:k].double().cpu()
        e = edges[:k].double().cpu()
        P64 = {name: p.detach().double().cpu() for name, p in self.A.state_dict().items()}
        with torch.no_grad():
            if self.kind == "MNN":
                ref = MO.mnn_forward(P64, self.cfg, n, e)
            else:
                ref = O.FORWARDS[self.kind](P64, self.cfg, n, e)
        got = out[:k].double().cpu()
        live = e.reshape(k, -1).any(1)
        if live.any():
            assert rel(got[live], ref[live]) < TOL
        assert rel(got, ref) < MASKED_TOL

    def check_done(self):
        if self.A.sync_free:
            self.A.last_bounded_error()
            self.B.last_bounded_error()


def poison(model):
    """Create the model's caches now and fill what a derivation must write with NaN."""
    probe = torch.zeros(1, model.constants.max_n_nodes, model.constants.n_node_features, device=DEV)
    params = model._params()
    if model.cache_weights:
        st = model._weights_cache(params, probe)
        st["buf"].fill_(float("nan"))
        assert not st["valid"]
    if model.cache_pass0:
        buf = model._pass0_cache(params, probe)
        n = buf.numel()
        assert (n - P0_ROWS_WORD) > 0 and (n - P0_ROWS_WORD) % (2 * L.GI_MAX_GROUPS * 256) == 0, n
        buf.zero_()
        buf[P0_ROWS_WORD:].view(torch.float32).fill_(float("nan"))
    torch.cuda.synchronize()


def batch(B, seed, shape=GDB13, **kw):
    n8, e8, _ = synthetic.make_batch(B, **shape, seed=seed, **kw)
    return torch.from_numpy(n8).float().to(DEV), torch.from_numpy(e8).float().to(DEV)


def edgeless(B, seed):
    """Atoms, no bonds."""
    nodes, edges = batch(B, seed)
    return nodes, torch.zeros_like(edges)


def single_atoms(B, seed):
    nodes, edges = batch(B, seed, frac_empty=0.0)
    nodes[:, 1:] = 0
    return nodes, torch.zeros_like(edges)


def one_bond(B, seed):
    """Empty graphs, except the first one: two atoms and one bond."""
    nodes, edges = batch(B, seed, frac_empty=0.0)
    nodes[1:] = 0
    nodes[0, 2:] = 0
    edges.zero_()
    edges[0, 0, 1, 0] = edges[0, 1, 0, 0] = 1
    return nodes, edges


# ---- edge count across calls --------------------------------------------------------------------------------------

ORDERS = {
    "edgeless_then_normal": ["edgeless", "normal", "normal"],
    "normal_then_edgeless": ["normal", "edgeless", "normal"],
    "alternating": ["edgeless", "normal", "edgeless", "normal", "edgeless", "normal"],
    "single_atoms_then_normal": ["single", "normal", "single", "normal"],
    "one_bond_then_normal": ["one_bond", "normal", "one_bond", "normal"],
}
MAKERS = {"edgeless": edgeless, "single": single_atoms, "one_bond": one_bond, "normal": lambda B, s: batch(B, s)}


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("kind", ["GGNN", "AttGGNN"])
@pytest.mark.parametrize("sync_free", [False, True])
def test_edge_count_across_calls(order, kind, sync_free):
    pair = Pair(kind, sync_free=sync_free)
    B = 300
    for i, what in enumerate(ORDERS[order]):
        nodes, edges = MAKERS[what](B, 40 + i)
        out = pair.forward(nodes, edges, what)
    pair.anchor(nodes, edges, out)
    pair.check_done()


# ---- batch size across calls --------------------------------------------------------------------------------------

@pytest.mark.parametrize("sizes", [(1, 1000, 1, 1000), (3, 4000)], ids=["1-1000-1-1000", "3-4000"])
@pytest.mark.parametrize("kind", ["GGNN", "AttGGNN"])
@pytest.mark.parametrize("sync_free", [False, True])
def test_batch_size_across_calls(sizes, kind, sync_free):
    pair = Pair(kind, sync_free=sync_free)
    for i, B in enumerate(sizes):
        nodes, edges = batch(B, 50 + i)
        out = pair.forward(nodes, edges, f"B={B}")
    pair.anchor(nodes, edges, out)
    pair.check_done()


# ---- arithmetic switches between the derive and the use --------------------------------------------------------------

@pytest.fixture
def arithmetic_switches():
    lib = L.load()
    prev = lib.gi_bf3_enable(-1), lib.gi_x2_enable(-1), lib.gi_b3p_enable(-1)
    try:
        yield lib
    finally:
        lib.gi_bf3_enable(prev[0]); lib.gi_x2_enable(prev[1]); lib.gi_b3p_enable(prev[2])


@pytest.mark.parametrize("switch", ["bf3", "x2", "b3p"])
@pytest.mark.parametrize("first", [0, 1], ids=["off_then_on", "on_then_off"])
@pytest.mark.parametrize("sync_free", [False, True])
def test_switch_flipped_between_derive_and_use(switch, first, sync_free, arithmetic_switches):
    lib = arithmetic_switches
    flip = {"bf3": lib.gi_bf3_enable, "x2": lib.gi_x2_enable, "b3p": lib.gi_b3p_enable}[switch]
    pair = Pair("GGNN", sync_free=sync_free)
    nodes, edges = batch(1000, 60)             # >= 2 560 node rows: the 16-bit-pipe launches are taken
    flip(first)
    pair.forward(nodes, edges, f"{switch}={first}, derive")
    pair.forward(nodes, edges, f"{switch}={first}, reuse")
    flip(1 - first)
    out = pair.forward(nodes, edges, f"{switch}={1 - first}")
    pair.forward(nodes, edges, f"{switch}={1 - first}, reuse")
    pair.anchor(nodes, edges, out)
    flip(first)
    pair.forward(nodes, edges, f"{switch}={first} again")
    pair.check_done()


@pytest.mark.parametrize("sync_free", [False, True])
def test_tripped_guard_then_reset(sync_free, arithmetic_switches):
    """no_x2 through the fp16x2 guard's trip flag (bf16x3 from the next forward on), then x2_guard_reset()."""
    pair = Pair("GGNN", sync_free=sync_free)
    nodes, edges = batch(1000, 61)
    pair.forward(nodes, edges, "fp16x2, derive")
    for m in (pair.A, pair.B):
        assert not m._x2_off()
        m._x2_guard_state(nodes.device)[2].value = 1
        assert m._x2_off()
    out = pair.forward(nodes, edges, "tripped")
    pair.forward(nodes, edges, "tripped, reuse")
    pair.anchor(nodes, edges, out)
    for m in (pair.A, pair.B):
        m.x2_guard_reset()
        assert not m._x2_off()
    pair.forward(nodes, edges, "reset")
    pair.forward(nodes, edges, "reset, reuse")
    pair.check_done()


# ---- model variants -----------------------------------------------------------------------------------------------

def _variant(name):
    """(kind, config, batch maker, sync-free bounds) of a model whose caches hold a different set of things."""
    g = (GDB13["n_atom_types"], GDB13["n_formal_charge"], GDB13["max_n_nodes"])
    plain = lambda B, s: batch(B, s)
    if name == "mnn":                        # node-level cells only (img_fx = -1), no pass-0 table
        return "MNN", MO.mnn_config(*g), plain, None
    if name == "wide_enn":                   # enn_hidden_dim = 300: chain-ineligible message stacks
        return "GGNN", O.shaped_config(*g, enn_hidden_dim=300), plain, None
    if name == "wide_h":                     # H = M = 256: the chains at their width limit
        return "GGNN", O.shaped_config(*g, hidden_node_features=256, message_size=256), plain, None
    if name == "implicit_h":                 # A = 432: the node-level stacks' last layer is wide
        from tests.test_dims_gpu import _implicit_h_batch
        cfg = O.make_config(n_node_features=19, n_edge_features=3, max_n_nodes=13, len_f_add_per_node=432,
                            len_f_conn_per_node=3)

        def implicit(B, s):
            n8, e8, _ = _implicit_h_batch(B, s)
            return torch.from_numpy(n8).float().to(DEV), torch.from_numpy(e8).float().to(DEV)
        # up to 12 x 3 x 4 feature classes per bond type: above ops.default_bounds' 64, within GI_P0_MAX_CLASSES
        return "GGNN", cfg, implicit, (4 * 1000 * 13, 256 * 3)
    if name == "depth0":                     # every stack one Linear: pass-0 class rows produce the messages directly
        return "GGNN", O.shaped_config(*g, enn_depth=0, gather_att_depth=0, gather_emb_depth=0, mlp1_depth=0,
                                       mlp2_depth=0), plain, None
    if name == "passes1":                    # pass 0 is the only pass: the table's rows are the whole message stage
        return "GGNN", O.shaped_config(*g, message_passes=1), plain, None
    if name == "chain_maxl":                 # 8-layer message stacks (GI_CHAIN_MAXL): the largest chain image
        return "GGNN", O.shaped_config(*g, enn_depth=7), plain, None
    if name == "chain_over":                 # 9 layers: chain-ineligible by depth, layer by layer, no chain image
        return "GGNN", O.shaped_config(*g, enn_depth=8), plain, None
    if name == "narrow_readout":             # every node-level layer below BF3_MIN_WIDTH: no 16-bit-pipe launch
        return "GGNN", O.shaped_config(*g, gather_att_hidden_dim=160, gather_emb_hidden_dim=160,
                                       mlp1_hidden_dim=160, mlp2_hidden_dim=160), plain, None
    if name in ("ggnn_r2_r1", "att_r2_r1", "mnn_r2_r1"):    # widths that are no multiple of 4: padded images and cells
        from tests.test_widths_gpu import CASES, config
        kind, over = CASES[name]
        return kind, config(kind, over), plain, None
    raise KeyError(name)


@pytest.mark.parametrize("name", ["mnn", "wide_enn", "wide_h", "implicit_h", "narrow_readout", "depth0", "passes1",
                                  "chain_maxl", "chain_over", "ggnn_r2_r1", "att_r2_r1", "mnn_r2_r1"])
@pytest.mark.parametrize("sync_free", [False, True])
def test_model_variants(name, sync_free):
    kind, cfg, make, bounds = _variant(name)
    pair = Pair(kind, cfg=cfg, sync_free=sync_free, bounds=bounds)
    for i, (B, bonds) in enumerate([(1, True), (400, False), (1000, True), (2, True), (1000, True)]):
        nodes, edges = make(B, 70 + i)
        if not bonds:
            edges = torch.zeros_like(edges)
        out = pair.forward(nodes, edges, f"B={B}" + ("" if bonds else " edgeless"))
    pair.anchor(nodes, edges, out)
    pair.check_done()


# ---- weight-change routes between forwards ------------------------------------------------------------------------

def _train_step_grads(model, nodes, edges):
    model.train()
    model.zero_grad(set_to_none=True)
    model(nodes, edges).square().mean().backward()
    model.eval()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("sync_free", [False, True])
def test_torch_adam_step(sync_free):
    pair = Pair("GGNN", sync_free=sync_free)
    nodes, edges = batch(500, 80)
    before = pair.forward(nodes, edges, "derive")
    opt = torch.optim.Adam(pair.A.parameters(), lr=1e-2)
    _train_step_grads(pair.A, nodes, edges)
    opt.step()
    pair.sync_b()
    out = pair.forward(nodes, edges, "after Adam.step")
    assert not torch.equal(out, before)
    pair.forward(nodes, edges, "reuse")
    pair.anchor(nodes, edges, out)
    pair.check_done()


def test_data_parallel_broadcast_parameters():
    """gloo, world size 1, always_reduce: the broadcast runs.  The new weights are written through p.data, which no
    version counter sees, so only the broadcast's lib.WEIGHTS_EPOCH bump can tell the caches."""
    import torch.distributed as dist
    from graphinvent_amd import dp
    pair = Pair("GGNN")
    nodes, edges = batch(500, 81)
    before = pair.forward(nodes, edges, "derive")
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1)
    try:
        tr = dp.DataParallel(pair.A, torch.optim.SGD(pair.A.parameters(), lr=1e-3), always_reduce=True)
        g = torch.Generator(device=DEV).manual_seed(5)
        for p in pair.A.parameters():
            p.data.add_(torch.randn(p.shape, device=DEV, generator=g), alpha=1e-2 * float(p.detach().abs().max()))
        epoch = L.WEIGHTS_EPOCH[0]
        tr.broadcast_parameters(src=0)
        assert L.WEIGHTS_EPOCH[0] == epoch + 1
    finally:
        dist.destroy_process_group()
    pair.sync_b()
    out = pair.forward(nodes, edges, "after broadcast_parameters")
    assert not torch.equal(out, before)
    pair.forward(nodes, edges, "reuse")
    pair.anchor(nodes, edges, out)


@pytest.mark.parametrize("sync_free", [False, True])
def test_p_data_write_then_reset(sync_free):
    pair = Pair("GGNN", sync_free=sync_free)
    nodes, edges = batch(500, 82)
    before = pair.forward(nodes, edges, "derive")
    pair.forward(nodes, edges, "reuse")
    for name, p in pair.A.named_parameters():
        if name.startswith(("msg_nns.", "APDReadout.fAddNet1.")):
            p.data.mul_(0.75)
    pair.A.reset_pass0_cache()
    pair.sync_b()
    out = pair.forward(nodes, edges, "after p.data write + reset_pass0_cache")
    assert not torch.equal(out, before)
    pair.forward(nodes, edges, "reuse")
    pair.anchor(nodes, edges, out)
    pair.check_done()


@pytest.mark.parametrize("sync_free", [False, True])
def test_deepcopy_of_a_warm_model(sync_free):
    """The RL agent / prior pattern: a copy of a model whose caches are warm; the copy is trained, both are used in
    turn and each keeps serving its own weights."""
    pair = Pair("GGNN", sync_free=sync_free)
    nodes, edges = batch(500, 83)
    pair.forward(nodes, edges, "derive")
    pair.forward(nodes, edges, "reuse")
    agent = Pair.__new__(Pair)
    agent.kind, agent.cfg, agent.n = pair.kind, pair.cfg, 0
    agent.A, agent.B = copy.deepcopy(pair.A), copy.deepcopy(pair.B)
    poison(agent.A)
    a0 = agent.forward(nodes, edges, "copy, derive")
    assert torch.equal(a0, pair.forward(nodes, edges, "prior"))
    opt = torch.optim.Adam(agent.A.parameters(), lr=1e-2)
    _train_step_grads(agent.A, nodes, edges)
    opt.step()
    agent.sync_b()
    for _ in range(2):
        prior = pair.forward(nodes, edges, "prior")
        out = agent.forward(nodes, edges, "trained copy")
        assert not torch.equal(out, prior)
    assert torch.equal(prior, a0)
    pair.anchor(nodes, edges, prior)
    agent.anchor(nodes, edges, out)
    pair.check_done()
    agent.check_done()


# ---- mixed calls --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["GGNN", "AttGGNN"])
@pytest.mark.parametrize("sync_free", [False, True])
def test_training_forwards_in_between(kind, sync_free):
    """A training forward + backward, a train()-mode forward with dropout, a forward with grad enabled and no backward:
    none of them may disturb the caches of the no-grad forwards around them."""
    drop = dict(mlp1_dropout_p=0.1, mlp2_dropout_p=0.1)
    if kind == "AttGGNN":
        drop.update(msg_dropout_p=0.1, att_dropout_p=0.1)
    else:
        drop.update(enn_dropout_p=0.1)
    cfg = O.shaped_config(GDB13["n_atom_types"], GDB13["n_formal_charge"], GDB13["max_n_nodes"], **drop)
    pair = Pair(kind, cfg=cfg, sync_free=sync_free)
    nodes, edges = batch(500, 84)
    other = batch(700, 85)
    pair.forward(nodes, edges, "derive")
    for m in (pair.A, pair.B):                                  # (1) training forward + backward (dropout active)
        m.dropout_seed = 1234
        _train_step_grads(m, *other)
    pair.forward(nodes, edges, "after a training step")
    for m in (pair.A, pair.B):                                  # (2) train()-mode forward with dropout, no backward
        m.train()
        with torch.no_grad():
            m(*other)
        m.eval()
    pair.forward(*other, "after a dropout forward")
    for m in (pair.A, pair.B):                                  # (3) grad enabled, eval(), no backward
        out = m(*other)
        assert out.requires_grad
        del out
    out = pair.forward(nodes, edges, "after a grad-enabled forward")
    pair.anchor(nodes, edges, out)
    pair.check_done()


# ---- a failing call -----------------------------------------------------------------------------------------------

class _FailOnce:
    """The loaded library, except that its next gi_ggnn_forward_ex returns GI_EINVAL without launching anything."""

    def __init__(self, lib):
        self._lib, self.armed, self.failed = lib, True, 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "gi_ggnn_forward_ex":
            return fn

        def call(*args):
            if self.armed:
                self.armed = False
                self.failed += 1
                return -1                                     # GI_EINVAL
            return fn(*args)
        return call


@pytest.mark.parametrize("sync_free", [False, True])
def test_a_failed_forward_leaves_the_cache_underived(sync_free, monkeypatch):
    pair = Pair("GGNN", sync_free=sync_free)
    nodes, edges = batch(500, 86)
    proxy = _FailOnce(L.load())
    monkeypatch.setattr(L, "load", lambda: proxy)
    with torch.no_grad(), pytest.raises(RuntimeError, match="GI_EINVAL"):
        pair.A(nodes, edges)
    assert proxy.failed == 1
    assert not pair.A.__dict__["_w_state"]["valid"]
    out = pair.forward(nodes, edges, "after the failed call")
    pair.forward(nodes, edges, "reuse")
    pair.anchor(nodes, edges, out)
    pair.check_done()


# ---- capture across a weight update -------------------------------------------------------------------------------

def test_build_graphs_recaptures_after_a_weight_update(golden_dir):
    """build_graphs(capture=True) records its round again on every call: after a FusedAdam step the captured loop builds
    what the blocking loop builds with the new weights and the same uniforms."""
    from graphinvent_amd.generator import build_graphs
    from graphinvent_amd.optim import FusedAdam
    from oracle import callers_oracle as CO
    from tests.test_grow_gpu import STATE, _ggnn_generator, snapshot

    G, consts, model, u = _ggnn_generator(golden_dir)
    poison(model)

    def run(capture):
        gen = CO.GeneratorOracle(model, int(G["batch"]), consts, None)
        n = build_graphs(gen, consts.dim_f_add, consts.dim_f_conn, uniforms=u, capture=capture)
        torch.cuda.synchronize()
        return n, gen.generation_rounds, snapshot(gen)

    first = run(True)
    assert first[0] == int(G["n_generated"])
    nodes, edges = (torch.from_numpy(G[k]).float().to(DEV)[:64] for k in ("nodes", "edges"))
    opt = FusedAdam(model.parameters(), lr=5e-2)
    _train_step_grads(model, nodes, edges)
    epoch = L.WEIGHTS_EPOCH[0]
    opt.step()
    assert L.WEIGHTS_EPOCH[0] != epoch
    captured = run(True)
    blocking = run(False)
    assert captured[:2] == blocking[:2]
    for k in STATE:
        if k.endswith("likelihoods"):
            assert rel(captured[2][k], blocking[2][k]) < 1e-6, k
        else:
            assert torch.equal(captured[2][k], blocking[2][k]), k
    # the update reached the graphs: the likelihoods moved
    assert not torch.equal(captured[2]["generated_likelihoods"], first[2]["generated_likelihoods"])
