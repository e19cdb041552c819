"""CPU: the compiled-in limits of the HIP model and chain kernels, host side only (no device compute is issued).

The reference accepts any depth, pass count, graph size and number of bond types; the HIP model supports stack
depths 0..11, 0..16 message passes, max_n_nodes <= GI_MAX_NODES and n_edge_features <= GI_MAX_GROUPS
(csrc/gi_model.hip build_model).  Past a limit the model must refuse at construction, naming the limit; the C ABI
answers GI_ELIMIT, as include/graphinvent_amd.h documents.  Widths below 4 floats (one 16-byte vector) are refused at
construction too, for every width that is some layer's fan-in."""
import ctypes as C

import pytest
import torch

from graphinvent_amd import lib as L
from graphinvent_amd.gnn import mpnn
from oracle import ggnn_oracle as O
from tests import mnn_oracle as MO
from tests.golden.spec import TINY, TINY_ATT

GGNN_DEPTHS = ("enn_depth", "gather_att_depth", "gather_emb_depth", "mlp1_depth", "mlp2_depth")


def _dims(cfg, kind=L.KIND_GGNN):
    consts = MO.as_constants(cfg) if kind == L.KIND_MNN else O.as_constants(cfg)
    return mpnn._dims_from_constants(consts, 8, kind)


def test_the_deepest_accepted_models_have_a_full_parameter_table():
    """Every stack 11 deep and 16 passes builds, for the largest bond-type count too; the driver's parameter tables
    (slab plan, reduction lists) are sized for them: the slab plan of the backward is computed, not refused."""
    lib = L.load()
    deep = {k: L.MODEL_MAX_DEPTH for k in GGNN_DEPTHS}
    for model, kind, extra in (("GGNN", L.KIND_GGNN, {}),
                               ("AttGGNN", L.KIND_ATTGGNN, dict(msg_depth=L.MODEL_MAX_DEPTH, att_depth=L.MODEL_MAX_DEPTH))):
        for fe in (3, L.GI_MAX_GROUPS):
            cfg = O.make_config(**dict(TINY_ATT if model == "AttGGNN" else TINY, **deep, **extra,
                                       message_passes=L.MODEL_MAX_PASSES, n_edge_features=fe))
            d = _dims(cfg, kind)
            n = lib.gi_ggnn_num_params(C.byref(d))
            assert n == len(O.param_shapes(cfg, model)), (model, fe, n)
            Ut = (C.c_int * fe)(*([10] * fe))
            assert lib.gi_ggnn_slab_floats(C.byref(d), 40, 10 * fe, Ut) > 0, (model, fe)
            cls = mpnn.AttentionGGNN if model == "AttGGNN" else mpnn.GGNN
            m = cls(O.as_constants(cfg))
            assert [k for k, _ in m.named_parameters()] == list(O.param_shapes(cfg, model))


@pytest.mark.parametrize("key,value", [(k, L.MODEL_MAX_DEPTH + 1) for k in GGNN_DEPTHS] +
                         [("message_passes", L.MODEL_MAX_PASSES + 1), ("max_n_nodes", L.GI_MAX_NODES + 1),
                          ("n_edge_features", L.GI_MAX_GROUPS + 1)])
def test_ggnn_past_a_limit_fails_at_construction_naming_it(key, value):
    cfg = O.make_config(**dict(TINY, **{key: value}))
    with pytest.raises(ValueError, match=rf"{key} = {value}: .* from \d+ to {value - 1}"):
        mpnn.GGNN(O.as_constants(cfg))
    assert L.load().gi_ggnn_num_params(C.byref(_dims(cfg))) == -2           # GI_ELIMIT
    ok = O.make_config(**dict(TINY, **{key: value - 1}))                     # the limit itself builds
    mpnn.GGNN(O.as_constants(ok))
    assert L.load().gi_ggnn_num_params(C.byref(_dims(ok))) == len(O.param_shapes(ok))


@pytest.mark.parametrize("key", ["msg_depth", "att_depth"])
def test_attggnn_past_a_depth_limit_fails_at_construction(key):
    cfg = O.make_config(**dict(TINY_ATT, **{key: L.MODEL_MAX_DEPTH + 1}))
    with pytest.raises(ValueError, match=rf"{key} = 12: .* from 0 to 11"):
        mpnn.AttentionGGNN(O.as_constants(cfg))
    assert L.load().gi_ggnn_num_params(C.byref(_dims(cfg, L.KIND_ATTGGNN))) == -2


@pytest.mark.parametrize("key,value", [("mlp1_depth", 12), ("mlp2_depth", 12), ("message_passes", 17)])
def test_mnn_past_a_limit_fails_at_construction(key, value):
    cfg = MO.tiny_config(**{key: value})
    with pytest.raises(ValueError, match=rf"{key} = {value}: "):
        mpnn.MNN(MO.as_constants(cfg))
    assert L.load().gi_ggnn_num_params(C.byref(_dims(cfg, L.KIND_MNN))) == -2


WIDTH_KEYS = {
    "GGNN": [("hidden_node_features", None), ("message_size", None), ("gather_width", None),
             ("enn_hidden_dim", "enn_depth"), ("gather_att_hidden_dim", "gather_att_depth"),
             ("gather_emb_hidden_dim", "gather_emb_depth"), ("mlp1_hidden_dim", "mlp1_depth"),
             ("mlp2_hidden_dim", "mlp2_depth")],
    "AttGGNN": [("hidden_node_features", None), ("message_size", None), ("gather_width", None),
                ("msg_hidden_dim", "msg_depth"), ("att_hidden_dim", "att_depth"),
                ("gather_att_hidden_dim", "gather_att_depth"), ("gather_emb_hidden_dim", "gather_emb_depth"),
                ("mlp1_hidden_dim", "mlp1_depth"), ("mlp2_hidden_dim", "mlp2_depth")],
    "MNN": [("hidden_node_features", None), ("message_size", None), ("mlp1_hidden_dim", "mlp1_depth"),
            ("mlp2_hidden_dim", "mlp2_depth")],
}


@pytest.mark.parametrize("model,key,depth", [(m, k, d) for m, keys in WIDTH_KEYS.items() for k, d in keys])
def test_a_width_below_one_vector_fails_at_construction_naming_it(model, key, depth):
    """Widths of 1 to 3 (the reference accepts them) are the row length of a weight matrix that the GEMM family reads
    as stored, in 16-byte vectors: refused when the model is built, for every such key; 4 builds, and so does a
    narrower hidden width of a stack without hidden layers (depth 0), which never uses it."""
    if model == "MNN":
        cls, make, consts = mpnn.MNN, lambda **kw: MO.tiny_config(**kw), MO.as_constants
    else:
        cls = mpnn.AttentionGGNN if model == "AttGGNN" else mpnn.GGNN
        make = lambda **kw: O.make_config(**dict(TINY_ATT if model == "AttGGNN" else TINY, **kw))
        consts = O.as_constants
    for v in (1, 2, 3):
        with pytest.raises(ValueError, match=rf"{key} = {v}: .* at least 4"):
            cls(consts(make(**{key: v})))
    if key != "hidden_node_features":                          # (H >= n_node_features, which the tiny configs set to 5)
        cls(consts(make(**{key: 4})))
    if depth is not None:
        cls(consts(make(**{key: 1, depth: 0})))


def test_chain_longer_than_its_layer_limit_is_a_limit_error():
    """include/graphinvent_amd.h: nlayers <= GI_CHAIN_MAXL, GI_ELIMIT otherwise (callers then run the stack layer by
    layer); a chain of 0 layers stays a bad argument."""
    lib = L.load()
    p = L.ChainParams()
    p.ngroups, p.rows = 1, 64
    for l in range(L.CHAIN_MAXL):
        p.layer[l].K, p.layer[l].N = 100, 100
    p.nlayers = L.CHAIN_MAXL
    assert lib.gi_mlp_chain_image_floats(C.byref(p)) > 0
    p.nlayers = L.CHAIN_MAXL + 1
    assert lib.gi_mlp_chain_image_floats(C.byref(p)) == -2
    p.nlayers = 0
    assert lib.gi_mlp_chain_image_floats(C.byref(p)) == -1
