"""CPU: the argument checks of gi_ggnn_forward_ex and gi_ggnn_backward_phase, as a table of refused calls for the three
model kinds.  Every call here is refused before anything touches a device, so no device compute is issued; the
expected codes are the library's own at the commit before the forward and the backward got one shared call context,
kept as literals.

The base arguments of a row are complete (a call with them would be accepted and go on to the device): each row breaks
exactly what its name says, so the code it gets back belongs to that check."""
import ctypes as C

import pytest

from graphinvent_amd import lib as L

EINVAL = -1
KINDS = {"ggnn": L.KIND_GGNN, "attggnn": L.KIND_ATTGGNN, "mnn": L.KIND_MNN}
B, N, FN, FE, W, A, CC, PASSES = 2, 4, 5, 3, 16, 6, 3, 2
LDOUT = N * A + N * CC + 1
_BUF = (C.c_float * 64)()                 # stands in for every array: no refused call reads it
PTR = (C.addressof(_BUF) + 15) & ~15
_UT = (C.c_int * FE)(2, 2, 2)


def _dims(kind, dropout=0):
    d = L.GgnnDims()
    mnn = kind == L.KIND_MNN
    d.B, d.N, d.Fn, d.Fe, d.H, d.M, d.G, d.A, d.C, d.passes = B, N, FN, FE, W, W, W, A, CC, PASSES
    d.enn_depth = d.att_depth = d.emb_depth = 0 if mnn else 1
    d.enn_hidden = d.att_hidden = d.emb_hidden = d.mlp1_hidden = d.mlp2_hidden = d.eatt_hidden = W
    d.mlp1_depth = d.mlp2_depth = 1
    d.eatt_depth = 1 if kind == L.KIND_ATTGGNN else 0
    d.big_positive, d.kind, d.dropout, d.drop_seed = 1e6, kind, dropout, 7
    return d


def _graph(dropout=0):
    g = L.Graph()
    g.S, g.E, g.U = B * N, 6, 6
    for name in ("gfix", "u_src", "in_perm", "mu_off", "mu_dst", "mu_slot", "out_perm"):
        setattr(g, name, PTR)
    g.Ut = C.cast(_UT, C.POINTER(C.c_int))
    if not dropout:                       # (AlphaDropout training mode runs without the pass-0 class rows)
        g.D0, g.ldc0 = 3, 3
        for name in ("d_src", "cmat", "e2d", "cls_off", "cls_edges"):
            setattr(g, name, PTR)
    return g


class Args:
    """The complete arguments of one forward and one backward call of a kind."""

    def __init__(self, kind, dropout=0):
        self.dims, self.graph = _dims(kind, dropout), _graph(dropout)
        n = L.load().gi_ggnn_num_params(C.byref(self.dims))
        assert n > 0
        self.params = (C.c_void_p * n)(*([PTR] * n))
        self.grads = (C.c_void_p * n)(*([PTR] * n))
        self.ws = self.out = self.slabs = self.d_out = PTR
        self.ldout, self.flags, self.phase = LDOUT, 0, L.BWD_ALL
        self.no_dims = self.no_graph = False

    def forward(self):
        return L.load().gi_ggnn_forward_ex(None if self.no_dims else C.byref(self.dims), self.params,
                                           None if self.no_graph else C.byref(self.graph), self.ws, self.out,
                                           self.ldout, None, None, self.flags)

    def backward(self):
        return L.load().gi_ggnn_backward_phase(None if self.no_dims else C.byref(self.dims), self.params,
                                               None if self.no_graph else C.byref(self.graph), self.ws, self.slabs,
                                               self.out, self.ldout, self.d_out, LDOUT, self.grads, None, None,
                                               self.phase)


def _set(**fields):
    def edit(a):
        for k, v in fields.items():
            setattr(a, k, v)
    return edit


def _gset(**fields):
    def edit(a):
        for k, v in fields.items():
            setattr(a.graph, k, v)
    return edit


ALL, CLASS_ROWS, FWD, BWD, BOTH = ("ggnn", "attggnn", "mnn"), ("ggnn", "attggnn"), ("forward",), ("backward",), \
    ("forward", "backward")
# (name, calls, kinds, dropout mode, edit of the complete arguments, expected code)
ROWS = [
    ("null dims", BOTH, ALL, 0, _set(no_dims=True), EINVAL),
    ("null graph", BOTH, ALL, 0, _set(no_graph=True), EINVAL),
    ("null params", BOTH, ALL, 0, _set(params=None), EINVAL),
    ("null ws", BOTH, ALL, 0, _set(ws=None), EINVAL),
    ("null out", BOTH, ALL, 0, _set(out=None), EINVAL),
    ("null slabs", BWD, ALL, 0, _set(slabs=None), EINVAL),
    ("null d_out", BWD, ALL, 0, _set(d_out=None), EINVAL),
    ("null grads", BWD, ALL, 0, _set(grads=None), EINVAL),
    ("null gfix", BOTH, ALL, 0, _gset(gfix=None), EINVAL),
    ("null Ut", BOTH, ALL, 0, _gset(Ut=None), EINVAL),
    ("unknown run flag", FWD, ALL, 0, _set(flags=4), EINVAL),
    ("unknown phase", BWD, ALL, 0, _set(phase=3), EINVAL),
    ("ldout one short", FWD, ALL, 0, _set(ldout=LDOUT - 1), EINVAL),
    ("U > E", BOTH, ALL, 0, _gset(E=5), EINVAL),
    ("E > 0 with U == 0", BOTH, ALL, 0, _gset(U=0, D0=0), EINVAL),
    ("E > 0 without u_src", BOTH, ALL, 0, _gset(u_src=None), EINVAL),
    ("E > 0 without in_perm", BOTH, ALL, 0, _gset(in_perm=None), EINVAL),
    ("E > 0 without mu_off", BWD, ALL, 0, _gset(mu_off=None), EINVAL),
    ("E > 0 without mu_dst", BWD, ALL, 0, _gset(mu_dst=None), EINVAL),
    ("E > 0 without out_perm", BWD, ALL, 0, _gset(out_perm=None), EINVAL),
    ("E > 0 without mu_slot", BWD, CLASS_ROWS, 0, _gset(mu_slot=None), EINVAL),
    ("D0 > U", BOTH, ALL, 0, _gset(D0=7, ldc0=7), EINVAL),
    ("D0 < 0", BOTH, ALL, 0, _gset(D0=-1), EINVAL),
    ("D0 > 0 without d_src", BOTH, CLASS_ROWS, 0, _gset(d_src=None), EINVAL),
    ("D0 > 0 without cmat", BOTH, CLASS_ROWS, 0, _gset(cmat=None), EINVAL),
    ("D0 > 0 with ldc0 < D0", BOTH, CLASS_ROWS, 0, _gset(ldc0=2), EINVAL),
    ("D0 > 0 without e2d", BOTH, ("attggnn",), 0, _gset(e2d=None), EINVAL),
    ("D0 > 0 without cls_off", BOTH, ("attggnn",), 0, _gset(cls_off=None), EINVAL),
    ("D0 > 0 without cls_edges", BOTH, ("attggnn",), 0, _gset(cls_edges=None), EINVAL),
    # (dropout mode needs D0 == 0, which a bounded GGNN / AttentionGGNN forward is refused for as well: only the MNN
    # case has this check to itself)
    ("bounded with dropout", FWD, ALL, 1, _gset(bounded=1), EINVAL),
    ("bounded with D0 == 0", FWD, CLASS_ROWS, 0, _gset(bounded=1, D0=0), EINVAL),
    ("wcache not 16-byte aligned", FWD, ALL, 0, _gset(wcache=PTR + 4), EINVAL),
    ("wcache in the backward", BWD, ALL, 0, _gset(wcache=PTR), EINVAL),
    ("bounded in the MNN backward", BWD, ("mnn",), 0, _gset(bounded=1), EINVAL),
    ("dropout with U != E", BOTH, ALL, 1, _gset(E=7), EINVAL),
    ("dropout with shared rows (S != B N)", BOTH, ALL, 1, _gset(S=B * N - 1), EINVAL),
    ("dropout with class rows", BOTH, ALL, 1, _gset(D0=3, ldc0=3, d_src=PTR, cmat=PTR, e2d=PTR, cls_off=PTR,
                                                    cls_edges=PTR), EINVAL),
]


@pytest.fixture(scope="module")
def switches_on():
    """the weights cache is looked at only with the 16-bit-pipe launches on (their defaults)"""
    lib = L.load()
    prev = (lib.gi_bf3_enable(1), lib.gi_x2_enable(1))
    yield
    lib.gi_bf3_enable(prev[0]); lib.gi_x2_enable(prev[1])


def test_the_base_arguments_are_well_formed():
    assert PTR % 16 == 0 and len(set(r[0] for r in ROWS)) == len(ROWS)
    for kind in KINDS.values():
        for dropout in (0, 1):
            a = Args(kind, dropout)
            ws = L.load().gi_ggnn_workspace_floats(C.byref(a.dims), a.graph.S, a.graph.E, a.graph.U, a.graph.D0)
            assert ws > 0                                 # dims and sizes pass the model's own checks


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_base_arguments_are_accepted_where_no_device_can_be_reached(kind, switches_on):
    """No refusal was added: the complete arguments get past every check and fail at the first HIP runtime call with
    HIP's no-device code.  Only asserted on a machine without a device (with one, the call would launch kernels on
    the stand-in buffer)."""
    import torch
    if torch.cuda.is_available():
        return
    for dropout in (0, 1):
        a = Args(KINDS[kind], dropout)
        assert a.forward() == 100 and a.backward() == 100, (kind, dropout)        # hipErrorNoDevice


CASES = [(row, kind) for row in ROWS for kind in KINDS if kind in row[2]]     # (a row names the kinds that make its check)


@pytest.mark.parametrize("row,kind", CASES, ids=[f"{r[0].replace(' ', '_')}-{k}" for r, k in CASES])
def test_refused_call(row, kind, switches_on):
    name, calls, kinds, dropout, edit, expected = row
    for call in calls:
        a = Args(KINDS[kind], dropout)
        edit(a)
        assert getattr(a, call)() == expected, (name, kind, call)
