"""-m gpu: log-likelihood of whole molecules (csrc/gi_loglik.hip, graphinvent_amd.likelihood).

1. The row kernels against fp64 numpy: widths from 1 to 9769, aligned and misaligned rows, two row pitches, logits
   scaled by 1 and 30, the special rows (hot at the ends, equal logits, -inf, +-80, NaN, hot = -1, hot = W).
2. The molecule sums bit for bit against the sequential fp32 sum in row order, however the rows are cut into launches.
3. molecule_log_likelihood end to end: the drop-in GGNN with the trained weights against golden_likelihood.npz (the
   unmodified reference), the torch restatement on the device's own logits, AttentionGGNN and MNN against their oracles.
4. Gradients against the golden ones; weighted_log_likelihood_backward against autograd.
5. No host synchronisation in the sync-free loop; invalid molecules; M = 0; a molecule of one atom."""
import numpy as np
import pytest
import torch

from graphinvent_amd import lib as L
from graphinvent_amd import likelihood as LL
from graphinvent_amd import ops, routes
from graphinvent_amd.gnn import mpnn
from oracle import ggnn_oracle as O
from tests import likelihood_model as LM
from tests import mnn_oracle as MO
from tests.test_likelihood_cpu import golden, golden_weights, oracle_logits, route_set

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -7.0


def _dev(x, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dtype)


def _err():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


# ---- 1 ------------------------------------------------------------------------------------------------------------

def _fp64(z, hot):
    """(ll, lse, p) in fp64; rows with hot == -1 give ll = lse = 0."""
    z = z.astype(np.float64)
    with np.errstate(all="ignore"):
        m = z.max(axis=1, keepdims=True)
        e = np.exp(z - m)
        s = e.sum(axis=1, keepdims=True)
        lse = (m + np.log(s))[:, 0]
        p = e / s
        ll = z[np.arange(z.shape[0]), np.clip(hot, 0, None)] - lse
    pad = hot < 0
    return np.where(pad, 0.0, ll), np.where(pad, 0.0, lse), p


def _row_kernel(view, hot, ll, lse, err):
    """gi_row_loglik itself, on outputs the caller filled."""
    rows, W = view.shape
    L.check(L.load().gi_row_loglik(view.data_ptr(), view.stride(0), rows, W, hot.data_ptr(), ll.data_ptr(),
                                   lse.data_ptr(), err.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()


def _assert_rows_close(got, ref):
    """The issue's bar, test_eval_gpu.py::test_kernel_against_fp64's: 1e-5 |ref| + 1e-6 per element."""
    assert np.isfinite(got).all()
    assert (np.abs(got - ref) <= 1e-5 * np.abs(ref) + 1e-6).all(), np.abs(got - ref).max()


def _assert_grad_close(d, g, p, hot, W):
    """d_logits against g (delta - p) in fp64.  Per element 2e-6 |g_r| + 1e-5 |ref|: the kernel's exp is v_exp_f32 on
    fl(x log2 e), a relative error of (1.2e-7 + 1.7e-7 |x|) on p = exp(x), i.e. at most 1.7e-7 max(p |ln p|) + 1.2e-7
    < 2e-7 absolute, twice (numerator and the renormalising sum) plus the roundings of delta - p and the product with
    g.  Every row sums to 0 within 1e-5 |g_r| (the issue's bar)."""
    rows = d.shape[0]
    ref = -p * g[:, None]
    live = hot >= 0
    ref[np.arange(rows)[live], hot[live]] += g[live]
    ref[~live] = 0
    assert (np.abs(d - ref) <= 2e-6 * np.abs(g)[:, None] + 1e-5 * np.abs(ref)).all(), np.abs(d - ref).max()
    assert (np.abs(d.astype(np.float64).sum(axis=1)) <= 1e-5 * np.abs(g)).all()
    assert (d[~live] == 0).all()


@pytest.mark.parametrize("W", [1, 2, 63, 64, 65, 625, 9769])
@pytest.mark.parametrize("rows", [1, 3, 257])
def test_row_kernels_against_fp64(W, rows):
    rng = np.random.default_rng(W * 1000 + rows)
    for pitch in (W, W + 3):
        for scale in (1.0, 30.0):
            buf = (rng.standard_normal((rows, pitch)) * scale).astype(np.float32)
            hot = rng.integers(0, W, rows).astype(np.int32)
            hot[0] = 0
            hot[-1] = W - 1
            ll64, lse64, p64 = _fp64(buf[:, :W], hot)
            view = _dev(buf)[:, :W]
            assert view.stride(0) == pitch
            logits = view.clone().requires_grad_(True) if pitch == W else view.detach().requires_grad_(True)
            err = _err()
            out = LL.row_log_likelihood(logits, _dev(hot), err)
            _assert_rows_close(out.detach().cpu().numpy(), ll64)
            ll = torch.full((rows,), SENTINEL, device=DEV)
            lse = torch.full((rows,), SENTINEL, device=DEV)
            _row_kernel(view, _dev(hot), ll, lse, err)
            assert torch.equal(ll, out.detach())                          # two runs bit for bit
            _assert_rows_close(lse.cpu().numpy(), lse64)
            g = (rng.standard_normal(rows) * 2).astype(np.float32)
            out.backward(_dev(g))
            assert int(err.item()) == 0
            _assert_grad_close(logits.grad.cpu().numpy(), g.astype(np.float64), p64, hot, W)


@pytest.mark.parametrize("W", [5, 65, 625])
def test_row_kernels_special_rows(W):
    NEG, NAN = -np.inf, np.nan
    rng = np.random.default_rng(W)
    kinds = ["first", "last", "equal", "only_hot", "hot_neg_inf", "pm80", "nan", "pad", "past_end", "below_pad",
             "plain"]
    rows = len(kinds)
    buf = (rng.standard_normal((rows, W + 3)) * 3).astype(np.float32)
    z = buf[:, :W]
    hot = rng.integers(0, W, rows).astype(np.int32)
    k = {name: i for i, name in enumerate(kinds)}
    hot[k["first"]], hot[k["last"]] = 0, W - 1
    z[k["equal"]] = 1.25
    z[k["only_hot"]] = NEG
    z[k["only_hot"], hot[k["only_hot"]]] = 3.5
    z[k["hot_neg_inf"], hot[k["hot_neg_inf"]]] = NEG
    z[k["pm80"]] = np.where(np.arange(W) % 2 == 0, 80.0, -80.0)
    z[k["nan"], (hot[k["nan"]] + 1) % W] = NAN
    hot[k["pad"]], hot[k["past_end"]], hot[k["below_pad"]] = -1, W, -2
    z[k["pad"]] = NAN                                                     # a padding row is not read
    ok = np.array([n not in ("past_end", "below_pad") for n in kinds])
    ll64, lse64, p64 = _fp64(z[ok], hot[ok])
    view, dhot, err = _dev(buf)[:, :W], _dev(hot), _err()
    ll = torch.full((rows,), SENTINEL, device=DEV)
    lse = torch.full((rows,), SENTINEL, device=DEV)
    _row_kernel(view, dhot, ll, lse, err)
    got = ll.cpu().numpy()
    assert int(err.item()) == L.LL_ERR_HOT
    assert (got[~ok] == SENTINEL).all() and (lse.cpu().numpy()[~ok] == SENTINEL).all()      # no write
    got_ok = dict(zip([n for n, o in zip(kinds, ok) if o], zip(got[ok], ll64)))
    for name in ("first", "last", "equal", "pm80", "plain"):
        a, b = got_ok[name]
        assert np.isfinite(a) and abs(a - b) <= 1e-5 * abs(b) + 1e-6, (name, a, b)
    assert abs(got_ok["equal"][0] + np.log(W)) <= 1e-5 * np.log(W) + 1e-6
    assert got_ok["only_hot"][0] == 0.0 and got_ok["only_hot"][1] == 0.0
    assert got_ok["hot_neg_inf"][0] == -np.inf and got_ok["hot_neg_inf"][1] == -np.inf
    assert np.isnan(got_ok["nan"][0]) and np.isnan(got_ok["nan"][1])
    assert got_ok["pad"][0] == 0.0 and lse.cpu().numpy()[k["pad"]] == 0.0
    # backward: the padding row and the two refused rows are exactly zero; -inf logits get exactly 0
    logits = view.detach().requires_grad_(True)
    err2 = _err()
    g = np.linspace(0.5, 2.0, rows).astype(np.float32)
    LL.row_log_likelihood(logits, dhot, err2).backward(_dev(g))
    d = logits.grad.cpu().numpy()
    assert int(err2.item()) == L.LL_ERR_HOT
    for name in ("pad", "past_end", "below_pad"):
        assert (d[k[name]] == 0).all(), name
    assert (d[k["only_hot"]] == 0).all()                                 # p = 1 at hot, 0 at every -inf logit
    r = k["hot_neg_inf"]
    assert d[r, hot[r]] == g[r] and np.isfinite(d[r]).all()              # delta - 0
    assert np.isnan(d[k["nan"]]).all()
    fin = np.array([n in ("first", "last", "equal", "pm80", "plain") for n in kinds])
    ll_f, _, p_f = _fp64(z[fin], hot[fin])
    _assert_grad_close(d[fin], g[fin].astype(np.float64), p_f, hot[fin], W)


def test_row_backward_takes_its_weight_from_the_molecule_and_the_kind():
    rows, W, M, n_add, n_conn = 23, 65, 4, 40, 24
    rng = np.random.default_rng(5)
    z = (rng.standard_normal((rows, W)) * 3).astype(np.float32)
    hot = rng.integers(0, W, rows).astype(np.int32)
    hot[:3] = [0, n_add, W - 1]
    row_mol = np.sort(rng.integers(0, M, rows)).astype(np.int32)
    row_mol[-2:] = -1
    g_mol = rng.standard_normal(M).astype(np.float32)
    g_kind = rng.standard_normal((M, 3)).astype(np.float32)
    _, lse64, p64 = _fp64(z, hot)
    dz, dhot, drm, err = _dev(z), _dev(hot), _dev(row_mol), _err()
    _, lse = LL._row_forward(dz, dhot, err)
    kind = (hot >= n_add).astype(int) + (hot >= n_add + n_conn).astype(int)
    for gk in (None, g_kind):
        g = g_mol[np.clip(row_mol, 0, None)].astype(np.float64)
        if gk is not None:
            g = (g_mol[np.clip(row_mol, 0, None)] + gk[np.clip(row_mol, 0, None), kind]).astype(np.float64)
        g[row_mol < 0] = 0
        d = LL._row_backward(dz, dhot, lse, _dev(g_mol), err, drm, None if gk is None else _dev(gk), n_add, n_conn)
        d = d.cpu().numpy()
        assert (d[row_mol < 0] == 0).all()
        _assert_grad_close(d, g, p64, hot, W)
    # a row_mol past the molecules: the bit, an exactly zero row, nothing indexed with it
    bad = row_mol.copy()
    bad[4] = M
    d = LL._row_backward(dz, dhot, lse, _dev(g_mol), err, _dev(bad)).cpu().numpy()
    assert int(err.item()) == L.LL_ERR_MOL and (d[4] == 0).all() and (d[5] != 0).any()


# ---- 2 ------------------------------------------------------------------------------------------------------------

def _sum_in_launches(rows_ll, hot, row_mol, M, cuts, n_add, n_conn, start=None, err=None):
    """mol_ll / mol_kind after one gi_mol_loglik_sum per piece [cuts[i], cuts[i + 1])."""
    mol = torch.zeros(M, device=DEV) if start is None else _dev(start)
    kind = torch.zeros((M, 3), device=DEV)
    err = _err() if err is None else err
    d_ll, d_hot, d_rm = _dev(rows_ll), _dev(hot), _dev(row_mol)
    for a, b in zip(cuts[:-1], cuts[1:]):
        if b > a:
            LL._mol_sum(d_ll[a:b], d_rm[a:b], d_hot[a:b], n_add + n_conn + 1, n_add, n_conn, mol, kind, err)
    torch.cuda.synchronize()
    return mol.cpu().numpy(), kind.cpu().numpy(), int(err.item())


def test_molecule_sums_do_not_depend_on_where_the_launches_cut():
    rng = np.random.default_rng(9)
    row_mol = np.array([0, 0, 0, 0, 1, 1, 2, 2, 2], np.int32)
    n_add, n_conn = 40, 24
    hot = rng.integers(0, 65, 9).astype(np.int32)
    hot[[0, 4, 6]] = 64
    rows_ll = (-np.exp(rng.standard_normal(9) * 2)).astype(np.float32)    # magnitudes that do not add exactly
    ref = LM.sequential_sum(rows_ll, row_mol, 3)
    ref_kind = LM.sequential_kinds(rows_ll, hot, row_mol, 3, n_add, n_conn)
    assert not np.array_equal(ref, rows_ll[[0, 4, 6]])
    cases = [[0, p, 9] for p in range(10)] + [list(range(10))]
    for cuts in cases:
        mol, kind, err = _sum_in_launches(rows_ll, hot, row_mol, 3, cuts, n_add, n_conn)
        assert err == 0
        assert np.array_equal(mol, ref), cuts                             # bit for bit
        assert np.array_equal(kind, ref_kind), cuts


def test_molecule_sums_of_long_routes_padding_rows_and_accumulation():
    rng = np.random.default_rng(10)
    row_mol = np.concatenate([np.full(2, 0), np.full(18, 1), [-1, -1], np.full(130, 3), [-1]]).astype(np.int32)
    R, M, n_add, n_conn = row_mol.shape[0], 5, 40, 24
    hot = rng.integers(0, 65, R).astype(np.int32)
    rows_ll = (-np.exp(rng.standard_normal(R))).astype(np.float32)
    rows_ll[row_mol < 0] = np.nan                                         # skipped, not added
    ref = LM.sequential_sum(rows_ll, row_mol, M)
    ref_kind = LM.sequential_kinds(rows_ll, hot, row_mol, M, n_add, n_conn)
    assert ref[2] == 0 and ref[4] == 0
    for cuts in ([0, R], [0, 75, R], [0, 1, 21, 22, 150, R]):
        mol, kind, err = _sum_in_launches(rows_ll, hot, row_mol, M, cuts, n_add, n_conn)
        assert err == 0 and np.array_equal(mol, ref) and np.array_equal(kind, ref_kind), cuts
    start = np.array([1.5, -2.0, 3.0, 0.25, 7.0], np.float32)             # += across calls
    mol, _, _ = _sum_in_launches(rows_ll, hot, row_mol, M, [0, R], n_add, n_conn, start=start)
    assert np.array_equal(mol, LM.sequential_sum(rows_ll, row_mol, M, start=start))


def test_molecule_sum_refuses_a_decreasing_row_mol_and_writes_nothing():
    rows_ll = np.array([-1.0, -2.0, -3.0, -4.0, -5.0], np.float32)
    hot = np.zeros(5, np.int32)
    start = np.full(3, SENTINEL, np.float32)
    for row_mol, bit in (([0, 0, 1, 0, 2], L.LL_ERR_ORDER), ([0, 1, -1, 0, 2], L.LL_ERR_ORDER),
                         ([0, 0, 1, 3, -1], L.LL_ERR_MOL), ([0, 0, -2, 1, 1], L.LL_ERR_MOL)):
        err = _err()
        row_mol = np.array(row_mol, np.int32)
        mol, kind, bits = _sum_in_launches(rows_ll, hot, row_mol, 3, [0, 5], 1, 1, start=start, err=err)
        assert bits == bit, (row_mol, bits)
        assert (mol == SENTINEL).all() and (kind == 0).all()
        # ... and neither does a later valid call while the bit is set
        mol, _, _ = _sum_in_launches(rows_ll, hot, np.array([0, 0, 1, 1, 2], np.int32), 3, [0, 5], 1, 1, start=start,
                                     err=err)
        assert (mol == SENTINEL).all()
    mol, _, bits = _sum_in_launches(rows_ll, hot, np.array([0, -1, 0, 1, -1], np.int32), 3, [0, 5], 1, 1)
    assert bits == 0 and np.array_equal(mol, np.array([-4.0, -4.0, 0.0], np.float32))


# ---- 3 ------------------------------------------------------------------------------------------------------------

class Recorder:
    """The model under test, keeping (a clone of) every chunk it saw and the logits it returned."""

    def __init__(self, model):
        self.model, self.seen = model, []

    def __call__(self, nodes, edges):
        out = self.model(nodes, edges)
        self.seen.append((nodes.clone(), edges.clone(), out.detach().clone()))
        return out

    def __getattr__(self, name):
        return getattr(self.__dict__["model"], name)


def _golden_model():
    cfg, P = golden_weights()
    model = mpnn.GGNN(O.as_constants(dict(cfg, device=DEV)))
    model.load_state_dict(P)
    return model.to(DEV).eval()


def _molecules(name="gdb13::"):
    _, _, _, _, mn, me, add, conn = route_set(name)
    return _dev(mn), _dev(me), add.tolist(), conn.tolist()


def _logit_slack(rec, ref_logits):
    """test_eval_gpu.py's: the logits bar (1e-4 of the largest reference magnitude) holds; how far the logits moved."""
    got = torch.cat([out for _, _, out in rec.seen]).cpu()
    assert got.shape == ref_logits.shape
    slack = float((got - ref_logits).abs().max())
    assert slack <= 1e-4 * float(ref_logits.abs().max()), slack
    return slack, got


def _assert_molecules_close(got, ref_rows, row_mol, slack, what=""):
    """Per molecule: the sum over its rows of test_eval_gpu.py's _assert_nll_close bound."""
    M = got.shape[0]
    bound = np.bincount(row_mol, weights=1e-4 + 1e-4 * np.abs(ref_rows) + 2 * slack, minlength=M)
    ref = np.bincount(row_mol, weights=ref_rows, minlength=M)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"\n{what} logits moved {slack:.2e}; molecule ll: max err {err.max():.2e}, smallest bound {bound.min():.2e}, "
          f"max err / bound {(err / bound).max():.3f}")
    assert np.isfinite(got).all() and (err <= bound).all()


@pytest.mark.parametrize("batch_rows", [1360, 256, 7])
def test_golden_molecules_end_to_end(batch_rows):
    G = golden()
    _, _, hot, row_mol = route_set()[:4]
    dn, de, add, conn = _molecules()
    n_add, n_conn = LM.kind_dims(add, conn)
    rec = Recorder(_golden_model())
    with torch.no_grad():
        ll, kind = LL.molecule_log_likelihood(rec, dn, de, add, conn, batch_rows=batch_rows, by_kind=True)
    assert ll.shape == (140,) and kind.shape == (140, 3) and ll.dtype == kind.dtype == torch.float32
    assert [s[0].shape[0] for s in rec.seen] == [min(batch_rows, 1360 - a) for a in range(0, 1360, batch_rows)]
    assert all(s[0].dtype == torch.int8 for s in rec.seen)
    slack, z = _logit_slack(rec, oracle_logits())
    got = ll.cpu().numpy()
    _assert_molecules_close(got, G["row_ll"], row_mol, slack, f"[batch_rows {batch_rows}]")
    got_kind = kind.cpu().numpy().astype(np.float64)
    kinds = LM.kind_of(torch.from_numpy(hot), n_add, n_conn).numpy()
    for c in range(3):                                                    # the same bound over the rows of one kind
        bound = np.bincount(row_mol, weights=(1e-4 + 1e-4 * np.abs(G["row_ll"]) + 2 * slack) * (kinds == c),
                            minlength=140)
        assert (np.abs(got_kind[:, c] - G["mol_kind"][:, c]) <= bound).all(), c
    # the restatement on the device's own logits
    h, rm = _dev(hot).long(), _dev(row_mol).long()
    rows64 = LM.row_ll(z.to(DEV).double(), h)
    ref = LM.molecule_ll(rows64, rm, 140)
    assert torch.allclose(ll.double(), ref, rtol=1e-6, atol=1e-6), float((ll.double() - ref).abs().max())
    ref_kind = LM.molecule_kinds(rows64, h, rm, 140, n_add, n_conn)
    assert torch.allclose(kind.double(), ref_kind, rtol=1e-6, atol=1e-6)


def _arom_model(kind, seed=3):
    _, _, _, _, mn, me, add, conn = route_set("arom5::")
    N, Fn, Fe = mn.shape[1], mn.shape[2], me.shape[3]
    shape = dict(n_node_features=Fn, n_edge_features=Fe, max_n_nodes=N,
                 len_f_add_per_node=int(np.prod(add[1:])), len_f_conn_per_node=Fe)
    if kind == "MNN":
        cfg = dict(MO.mnn_config(4, 3, N, Fe), **shape)
        P = MO.init_params(cfg, seed=seed)
        model = mpnn.MNN(MO.as_constants(dict(cfg, device=DEV)))
        forward = lambda n, e: MO.mnn_forward(P, cfg, n, e)
    else:
        cfg = O.make_config(**shape)
        P = O.init_params(cfg, seed=seed, model="AttGGNN")
        model = mpnn.AttentionGGNN(O.as_constants(dict(cfg, device=DEV)))
        forward = lambda n, e: O.attggnn_forward(P, cfg, n, e)
    model.load_state_dict(P)
    return model.to(DEV).eval(), forward


@pytest.mark.parametrize("kind", ["AttGGNN", "MNN"])
def test_other_models_at_four_bond_types_against_their_oracles(kind):
    rn, re_, hot, row_mol, mn, me, add, conn = route_set("arom5::")
    assert me.shape[3] == 4 and len(add) == 5
    model, forward = _arom_model(kind)
    with torch.no_grad():
        ref_logits = forward(torch.from_numpy(rn).float(), torch.from_numpy(re_).float())
    ref_rows = LM.row_ll(ref_logits.double(), torch.from_numpy(hot).long()).numpy()
    rec = Recorder(model)
    with torch.no_grad():
        ll = LL.molecule_log_likelihood(rec, _dev(mn), _dev(me), add.tolist(), conn.tolist(), batch_rows=100)
    slack, _ = _logit_slack(rec, ref_logits)
    _assert_molecules_close(ll.cpu().numpy(), ref_rows, row_mol, slack, f"[{kind}]")


# ---- 4 ------------------------------------------------------------------------------------------------------------

def _grad_errors(model, G):
    """rl_callers.grad_errors: (global relative L2, worst per-tensor max-abs relative) against the golden."""
    num = den = worst = 0.0
    for k, p in model.named_parameters():
        ref = torch.from_numpy(G["g::" + k]).double()
        got = p.grad.detach().double().cpu()
        num += float((got - ref).pow(2).sum())
        den += float(ref.pow(2).sum())
        worst = max(worst, float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-30)))
    return (num / den) ** 0.5, worst


def test_gradients_against_the_golden_and_the_streaming_backward():
    G = golden()
    dn, de, add, conn = _molecules()
    w = _dev(G["w"])
    model = _golden_model()
    ll = LL.molecule_log_likelihood(model, dn, de, add, conn, batch_rows=256)
    assert ll.requires_grad
    loss = -(w * ll).sum() / 140
    loss.backward()
    assert abs(float(loss.detach()) - float(G["loss"])) <= 1e-4 * abs(float(G["loss"]))
    l2, worst = _grad_errors(model, G)
    print(f"\nautograd vs the reference run: global L2 {l2:.2e}, worst tensor {worst:.2e}, loss "
          f"{float(loss.detach()):.6f} (reference {float(G['loss']):.6f})")
    assert l2 <= 5e-3 and worst <= 3e-2, (l2, worst)
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    model.zero_grad(set_to_none=True)
    ll2 = LL.weighted_log_likelihood_backward(model, dn, de, add, conn, -w / 140, batch_rows=256)
    assert not ll2.requires_grad and torch.allclose(ll2, ll.detach(), rtol=1e-6, atol=1e-6)
    for k, p in model.named_parameters():
        scale = float(grads[k].abs().max())
        assert float((p.grad - grads[k]).abs().max()) <= 1e-5 * scale, k
    # it accumulates: a second pass doubles the gradients
    LL.weighted_log_likelihood_backward(model, dn, de, add, conn, -w / 140, batch_rows=256)
    for k, p in model.named_parameters():
        assert torch.allclose(p.grad, 2 * grads[k], rtol=1e-4, atol=1e-5 * float(grads[k].abs().max())), k


def test_by_kind_is_differentiable_too():
    dn, de, add, conn = _molecules()
    model = _golden_model()
    c = torch.tensor([0.5, -1.0, 2.0], device=DEV)
    ll, kind = LL.molecule_log_likelihood(model, dn[:12], de[:12], add, conn, batch_rows=50, by_kind=True)
    assert torch.allclose(kind.sum(1), ll, rtol=1e-5, atol=1e-5)
    (kind * c).sum().backward()
    by_kind = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    model.zero_grad(set_to_none=True)
    # the restatement's gradient of the same objective with respect to the logits, pushed through the model once
    rec = Recorder(model)
    ll2 = LL.molecule_log_likelihood(rec, dn[:12], de[:12], add, conn, batch_rows=1000)
    n_add, n_conn = LM.kind_dims(add, conn)
    _, _, hot, row_mol = route_set()[:4]
    rows = row_mol < 12
    z = rec.seen[0][2].clone().requires_grad_(True)
    h, rm = _dev(hot[rows]).long(), _dev(row_mol[rows]).long()
    obj = (LM.molecule_kinds(LM.row_ll(z, h), h, rm, 12, n_add, n_conn) * c).sum()
    (dz,) = torch.autograd.grad(obj, z)
    model.zero_grad(set_to_none=True)
    out = model(rec.seen[0][0], rec.seen[0][1])
    out.backward(dz)
    for k, p in model.named_parameters():
        scale = float(p.grad.abs().max())
        assert float((by_kind[k] - p.grad).abs().max()) <= 1e-3 * scale + 1e-7, k
    assert ll2.requires_grad


# ---- 5 ------------------------------------------------------------------------------------------------------------

def _sync_debug_honoured() -> bool:
    torch.cuda.set_sync_debug_mode("error")
    try:
        torch.ones(1, device=DEV).item()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode(0)


def test_sync_free_loop_has_no_host_sync():
    _, _, _, _, mn, me, add, conn = route_set()
    dn, de = _dev(mn), _dev(me)
    n_rows = int(routes.route_lengths(mn, me).sum())
    assert n_rows == 1360
    model = _golden_model()
    with torch.no_grad():
        ref = LL.molecule_log_likelihood(model, dn, de, add.tolist(), conn.tolist(), batch_rows=400)
        model.sync_free = True
        LL.molecule_log_likelihood(model, dn, de, add.tolist(), conn.tolist(), batch_rows=400, n_rows=n_rows)
        torch.cuda.synchronize()                                   # first use allocated the sticky words
        strict = _sync_debug_honoured()
        print(f"\ntorch.cuda.set_sync_debug_mode honoured on this build: {strict}")
        before = dict(ops.READBACKS)
        if strict:
            torch.cuda.set_sync_debug_mode("error")
        try:
            ll = LL.molecule_log_likelihood(model, dn, de, add.tolist(), conn.tolist(), batch_rows=400, n_rows=n_rows)
        finally:
            torch.cuda.set_sync_debug_mode(0)
    delta = {k: ops.READBACKS[k] - before[k] for k in before}
    assert delta == {"prefetched": 0, "blocking": 0, "bounded": 4}, delta      # four forwards, none reads back
    assert torch.allclose(ll, ref, rtol=1e-5, atol=1e-5)
    with torch.no_grad(), pytest.raises(ValueError, match="rows"):
        LL.molecule_log_likelihood(model, dn, de, add.tolist(), conn.tolist(), batch_rows=400, n_rows=n_rows - 1)


def _broken(kind):
    """Three golden molecules, the middle one invalid in one way; the error bit."""
    from tests.test_routes_gpu import _break
    _, _, _, _, mn, me, _, _ = route_set()
    mn, me = mn[:3].copy(), me[:3].copy()
    if kind == "empty":
        mn[1], me[1] = 0, 0
        return mn, me, L.ROUTE_ERR_EMPTY
    if kind == "padding":
        mn[1], me[1] = 0, 0
        mn[1, 1, [0, 5]] = 1                                              # node 1 present, node 0 not
        return mn, me, L.ROUTE_ERR_PADDING
    return mn, me, _break(kind, mn, me)


@pytest.mark.parametrize("kind", ["no_lower_neighbour", "asymmetric", "two_bond_types", "not_one_hot", "not_0_1",
                                  "empty", "padding"])
def test_invalid_molecules_skip_or_raise(kind):
    _, _, _, _, gn, ge, add, conn = route_set()
    add, conn = add.tolist(), conn.tolist()
    mn, me, bit = _broken(kind)
    model = _golden_model()
    with torch.no_grad():
        good = LL.molecule_log_likelihood(model, _dev(gn[:3]), _dev(ge[:3]), add, conn)
        with pytest.raises(ValueError) as e:
            LL.molecule_log_likelihood(model, _dev(mn), _dev(me), add, conn)
        assert routes.ERROR_MESSAGES[bit] in str(e.value)
        with pytest.raises(ValueError) as e:                              # the same from the read-back after the loop
            LL.molecule_log_likelihood(model, _dev(mn), _dev(me), add, conn,
                                       n_rows=int(routes.route_lengths(gn[:3], ge[:3]).sum()))
        assert routes.ERROR_MESSAGES[bit] in str(e.value)
        ll, kinds, bits = LL.molecule_log_likelihood(model, _dev(mn), _dev(me), add, conn, invalid="skip",
                                                     by_kind=True)
    bits = bits.cpu().tolist()
    assert bits[0] == 0 and bits[2] == 0 and bits[1] & bit
    assert torch.isnan(ll[1]) and torch.isnan(kinds[1]).all()
    assert torch.allclose(ll[[0, 2]], good[[0, 2]], rtol=1e-4, atol=1e-4)


def test_no_molecules_and_a_molecule_of_one_atom():
    _, _, hot, row_mol, mn, me, add, conn = route_set()
    add, conn = add.tolist(), conn.tolist()
    model = _golden_model()
    with torch.no_grad():
        ll, kind = LL.molecule_log_likelihood(model, _dev(mn[:0]), _dev(me[:0]), add, conn, by_kind=True)
        assert ll.shape == (0,) and kind.shape == (0, 3) and ll.is_cuda and ll.dtype == torch.float32
        out = LL.molecule_log_likelihood(model, _dev(mn[:0]), _dev(me[:0]), add, conn, invalid="skip")
        assert out[0].shape == (0,) and out[1].shape == (0,) and out[1].dtype == torch.int32
        assert LL.weighted_log_likelihood_backward(model, _dev(mn[:0]), _dev(me[:0]), add, conn,
                                                   torch.zeros(0, device=DEV)).shape == (0,)
        one = int(np.where((mn.any(axis=2).sum(axis=1) == 1))[0][0])
        assert np.bincount(row_mol)[one] == 2                             # terminate-or-not on the atom, then the add
        rec = Recorder(model)
        ll = LL.molecule_log_likelihood(rec, _dev(mn[one:one + 1]), _dev(me[one:one + 1]), add, conn)
    assert ll.shape == (1,) and rec.seen[0][0].shape[0] == 2
    rows = LM.row_ll(rec.seen[0][2].double(), _dev(hot[row_mol == one]).long())
    assert abs(float(ll[0]) - float(rows.sum())) <= 1e-6 * abs(float(rows.sum())) + 1e-6
    G = golden()
    assert abs(float(ll[0]) - G["mol_ll"][one]) <= 2 * (1e-4 + 1e-4 * abs(G["mol_ll"][one]) + 2e-4 * 52.2)
