"""What constrained generation costs (informational; bench.py measures the flagship training workload).

    python tools/bench_constrained.py [--part round|mask|all] [--batch 1000] [--iters 50] [--repeats 15]
                                      [--parent-lib PATH] [--out FILE]

Run each part as its own command under its own time limit (``timeout -k 10 300 python tools/bench_constrained.py --part
round``).  Every variant is timed with device events over `--iters` calls, the variants ALTERNATING inside each of
`--repeats` repeats in one process; per variant the median and the min / max over the repeats.

  round   a whole generation round (forward, [mask,] draw, growth step) of the headline GGNN (reference defaults,
          h = 128, seeded weights, untrained) at B graphs, N = 13, on a FIXED batch of partly grown graphs (as
          tools/bench_seeded.py): ``unconstrained`` (constraint=None's path), ``constrained`` (the mask launch and
          the launch that keeps gen.constraint_stats) and, with --parent-lib (a libgraphinvent_amd.so built from the
          parent commit), ``parent_unconstrained``: the same round through that library;
  mask    the mask launch alone — fp32 and int8 states, one matrix and two — next to the sampler launch that follows
          it and a device copy of the logits it writes, at 1000 x 13 (A = 45), 250 x 88 (A = 432: W = 38281 is past the
          sampler's row limit, so the sampler is not measured there) and 1024 x 128 (A = 45).

Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from graphinvent_amd import analyze  # noqa: E402
from graphinvent_amd import lib as L  # noqa: E402
from graphinvent_amd import synthetic  # noqa: E402
from graphinvent_amd.generator import _STATE_TENSORS, _Grower, _Masker, new_state  # noqa: E402
from graphinvent_amd.gnn import mpnn  # noqa: E402
from graphinvent_amd.sampler import ActionConstraint, mask_actions_raw, sample_actions_raw  # noqa: E402
from oracle import ggnn_oracle as O  # noqa: E402
from tools.bench_generate import make_generator  # noqa: E402
from tools.bench_seeded import alternate  # noqa: E402

DEV = "cuda"
GDB13_TYPES, CHARGES = ["C", "N", "O", "S", "Cl"], [-1, 0, 1]
CHEMBL_TYPES = ["C", "N", "O", "F", "Si", "P", "S", "Cl", "Se", "Br", "I", "B"]


def parent_library(path):
    """The parent commit's library with this tree's prototypes (the symbols it lacks left out)."""
    lib = C.CDLL(os.path.abspath(path))
    for name, (res, args) in L.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


def bench_round(a):
    sh = synthetic.SHAPES["gdb13"]
    cfg = O.shaped_config(sh["n_atom_types"], sh["n_formal_charge"], sh["max_n_nodes"], hidden_node_features=128,
                          message_size=128)
    model = mpnn.GGNN(O.as_constants(dict(cfg, device=DEV)))
    model.load_state_dict(O.init_params(cfg, seed=0))
    model = model.to(DEV).eval()
    N, Fe = cfg["max_n_nodes"], cfg["n_edge_features"]
    groups = [sh["n_atom_types"], sh["n_formal_charge"]]
    d = dict(device=DEV, max_n_nodes=N, n_atom_types=groups[0], n_formal_charge=groups[1], n_imp_H=0,
             n_chirality=0, use_explicit_H=False, ignore_H=True, use_chirality=False, dim_nodes=[N, sum(groups)],
             dim_edges=[N, N, Fe], dim_f_add=[N, *groups, Fe], dim_f_conn=[N, Fe])
    c = namedtuple("CONSTANTS", sorted(d))(**d)
    rules = analyze.ValenceRules(GDB13_TYPES, CHARGES, bond_orders=(1, 2, 3), device=DEV)
    con = ActionConstraint(rules, c.dim_f_add, c.dim_f_conn)
    B, Lc = a.batch, 32
    g = torch.Generator(device=DEV).manual_seed(0)
    own = L.load()
    with torch.no_grad():
        gen = make_generator(model, B, c, Lc)
        t = {name: getattr(gen, name) for name, _ in _STATE_TENSORS}
        state = new_state(B, 10 ** 9, DEV)
        grower = _Grower(t, c.dim_f_add, c.dim_f_conn, state)
        masker = _Masker(con, t, state)
        for _ in range(a.prefill):                                         # constrained rounds: a batch of valid graphs
            u = torch.rand(B, device=DEV, generator=g)
            grower.step(*sample_actions_raw(masker.raw(model(gen.nodes, gen.edges)), gen.n_nodes, gen.edges, grower.A,
                                            uniform=u))
            state[0] = 0
        fixed = {k: v.clone() for k, v in t.items()}
        u = torch.rand(B, device=DEV, generator=g)

        def variant(constrained, lib):
            w = {k: v.clone() for k, v in fixed.items()}
            st = new_state(B, 10 ** 9, DEV)
            gr = _Grower(w, c.dim_f_add, c.dim_f_conn, st)
            mk = _Masker(con, fixed, st) if constrained else None

            def round_():
                L._lib = lib                                               # every call of the round goes through `lib`
                st[:2].zero_()
                z = model(fixed["nodes"], fixed["edges"])
                if mk is not None:
                    z = mk.raw(z)
                gr.step(*sample_actions_raw(z, fixed["n_nodes"], fixed["edges"], gr.A, uniform=u))
            return round_

        variants = {"unconstrained": variant(False, own), "constrained": variant(True, own)}
        if a.parent_lib:
            variants = {"parent_unconstrained": variant(False, parent_library(a.parent_lib)), **variants}
        try:
            out = alternate(variants, a.iters, a.repeats)
        finally:
            L._lib = own
    base = out["unconstrained"]
    out["constrained"]["ratio_to_unconstrained"] = round(out["constrained"]["median_ms"] / base["median_ms"], 4)
    if a.parent_lib:
        p = out["parent_unconstrained"]
        p["ratio_unconstrained_to_parent"] = round(base["median_ms"] / p["median_ms"], 4)
        p["inside_10_percent"] = bool(abs(base["median_ms"] / p["median_ms"] - 1.0) <= 0.10)
    return out


def random_states(rng, B, N, groups, Fe):
    """Well-formed states of 0 .. N atoms: random labels, sparse symmetric bonds, one type per pair."""
    nodes, edges = np.zeros((B, N, sum(groups)), np.int8), np.zeros((B, N, N, Fe), np.int8)
    n_nodes = rng.integers(0, N + 1, B)
    offs = np.concatenate([[0], np.cumsum(groups)[:-1]])
    for b in range(B):
        for i in range(n_nodes[b]):
            for off, size in zip(offs, groups):
                nodes[b, i, off + rng.integers(size)] = 1
            if i:
                j = rng.integers(i)
                edges[b, i, j, rng.integers(Fe)] = 1
        edges[b] |= edges[b].transpose(1, 0, 2)
    return nodes, edges, n_nodes


def bench_mask(a):
    out = {}
    shapes = {"1000x13": (1000, 13, GDB13_TYPES, None), "250x88": (250, 88, CHEMBL_TYPES, [0, 1, 2, 3]),
              "1024x128": (1024, 128, GDB13_TYPES, None)}
    rng = np.random.default_rng(0)
    g = torch.Generator(device=DEV).manual_seed(1)
    for name, (B, N, types, imp_h) in shapes.items():
        groups = [len(types), len(CHARGES)] + ([len(imp_h)] if imp_h else [])
        Fe = 3
        rules = analyze.ValenceRules(types, CHARGES, imp_H=imp_h, bond_orders=(1, 2, 3), allowed={("B", 1): (2,)},
                                     device=DEV)
        con = ActionConstraint(rules, [N, *groups, Fe], [N, Fe])
        nodes, edges, n_nodes = random_states(rng, B, N, groups, Fe)
        st = {"i8": (torch.from_numpy(nodes).to(DEV), torch.from_numpy(edges).to(DEV))}
        st["f32"] = tuple(x.float() for x in st["i8"])
        nn = torch.from_numpy(n_nodes).to(DEV, torch.int8 if N < 127 else torch.int32)
        z = torch.randn(B, con.W, device=DEV, generator=g)
        z2 = torch.randn(B, con.W, device=DEV, generator=g)
        u = torch.rand(B, device=DEV, generator=g)
        masked = mask_actions_raw(z, nn, *st["i8"], con)[0]
        dst = torch.empty_like(z)
        variants = {
            "mask_i8": lambda: mask_actions_raw(z, nn, *st["i8"], con, bits=False, removed=True),
            "mask_f32": lambda: mask_actions_raw(z, nn, *st["f32"], con, bits=False, removed=True),
            "mask_i8_two_matrices": lambda: mask_actions_raw(z, nn, *st["i8"], con, other=z2, bits=False, removed=True),
            "mask_i8_no_stats_with_bits": lambda: mask_actions_raw(z, nn, *st["i8"], con, bits=True, removed=False),
            "copy_of_the_logits": lambda: dst.copy_(z),
        }
        if con.W <= 15360:                                                  # the sampler's row limit
            variants["sampler"] = lambda: sample_actions_raw(masked, nn, st["i8"][1], con.A, uniform=u)
        res = alternate(variants, 4 * a.iters, a.repeats)
        if con.W > 15360:
            res["sampler"] = "not measured: W is past the sampler's row limit"
        res["W"], res["bytes_of_a_logits_matrix"] = con.W, 4 * B * con.W
        res["bytes_of_the_state"] = {k: int(v[0].numel() * v[0].element_size() + v[1].numel() * v[1].element_size())
                                     for k, v in st.items()}
        out[name] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("round", "mask", "all"), default="all")
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--prefill", type=int, default=6, help="constrained rounds that grow the fixed input batch")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_constrained.py needs an MI355X"
    out = {"batch": a.batch, "iters": a.iters, "repeats": a.repeats, "parent_lib": bool(a.parent_lib)}
    with torch.no_grad():
        if a.part in ("round", "all"):
            out["round"] = bench_round(a)
        if a.part in ("mask", "all"):
            out["mask"] = bench_mask(a)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
