"""Golden vectors of the generation loop's bookkeeping (tests/golden/golden_grow.npz), produced in the build container by
the UNMODIFIED reference ``GraphGenerator.build_graphs`` (GraphGenerator.py:99-161 with get_actions,
copy_terminated_graphs, apply_actions and reset_graphs) on CPU, imported through tests/golden/ref_callers.py.

``gen.model`` is tests/grow_oracle.py ``StubModel``: seeded random logits per call, regenerated from the seed on both
sides (not stored), biased per graph and round so that each run covers graph 0 drawing terminate, adds to full graphs,
connects on empty graphs (from = -1), duplicate bonds, several bond types gathering on graph 0, and terminated and
invalid graphs in one round.  The draw is pinned to ``InverseCdfDraws`` (ref_callers.pin_multinomial); seeds are picked
so that no draw came within 1e-4 of a CDF boundary, so an fp32 inverse-CDF draw on the device picks the same actions.

Three runs: add layouts atom type + charge (the first and the third) and atom type + charge + implicit H + chirality
(the first two branches of apply_actions, :264-301).  The third run's logits always add a node bonded to node 0, so no
graph finishes a second time before the reference runs out of likelihood columns and raises IndexError at round 2N;
its raising round is stored.

The reference reads the add's "from" as ``f_add_idc[5]`` in its full-graph check and its reset (:568, :617), which is
"from" only in the two-group layout (with implicit H and chirality it is the chirality index).  gi_sample_actions, like
oracle/sampler_oracle.py, takes the last index, so the implicit-H run is picked to stay clear of both places: no add
to a full graph (the reference would raise at :263) and every add with chirality 0 (what :568 resets it to).

Before anything is written, tests/grow_oracle.py ``run_oracle`` must reproduce every run bit for bit."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import callers_oracle as CO            # noqa: E402
from oracle import ggnn_oracle as O                # noqa: E402
from tests import grow_oracle as GO                # noqa: E402
from tests.golden import ref_callers as RC         # noqa: E402

MIN_MARGIN = 1e-4
BASE = dict(noise=1.0, drop=30.0, graph0_terminate_round=1)
CONFIGS = {
    "atoms_charges": dict(BASE, N=5, groups=[4, 3], Fe=3, B=32, ignore_H=1, use_chirality=0,
                          mode_p=[0.8, 0.05, 0.1, 0.05]),
    "imp_h_chirality": dict(BASE, N=6, groups=[3, 2, 3, 2], Fe=2, B=40, ignore_H=0, use_chirality=1,
                            mode_p=[0.88, 0.02, 0.07, 0.03], last_group_zero=1),
    "index_error": dict(BASE, N=4, groups=[3, 2], Fe=3, B=16, ignore_H=1, use_chirality=0,
                        mode_p=[1.0, 0.0, 0.0, 0.0], graph0_terminate_round=-1),
}
STATE = ("nodes", "edges", "n_nodes", "likelihoods", "generated_nodes", "generated_edges", "generated_n_nodes",
         "generated_likelihoods", "properly_terminated")


def constants(cfg):
    N, groups, Fe, dim_f_add, dim_f_conn = GO.config_dims(cfg)
    d = RC.constants_dict("cpu", O.make_config(), "/nonexistent", batch_size=int(cfg["B"]), epochs=1)
    imp_h = groups[2] if not cfg["ignore_H"] else 0
    chir = groups[-1] if cfg["use_chirality"] else 0
    d.update(max_n_nodes=N, n_atom_types=groups[0], n_formal_charge=groups[1], n_imp_H=imp_h, n_chirality=chir,
             n_edge_features=Fe, n_node_features=sum(groups), dim_nodes=[N, sum(groups)], dim_edges=[N, N, Fe],
             dim_f_add=dim_f_add, dim_f_conn=dim_f_conn, use_explicit_H=False, ignore_H=bool(cfg["ignore_H"]),
             use_chirality=bool(cfg["use_chirality"]))
    return RC.as_constants(d)


def pick_seeds(name, cfg):
    """First (stub_seed, draw_seed) whose oracle run has margin > MIN_MARGIN and covers every case."""
    for seed in range(1, 400):
        c = dict(cfg, stub_seed=seed, draw_seed=1000 + seed)
        s, draw, cover = GO.run_oracle(c)
        if draw.margin <= MIN_MARGIN:
            continue
        if name == "index_error":
            if s["error"] == GO.ERR_ROUND and s["round"] == 2 * int(c["N"]):
                return c, cover
            continue
        clear = name != "imp_h_chirality" or cover["add_to_full"] == 0     # (see the module docstring)
        need = [k for k in cover if k != "add_to_full" or name != "imp_h_chirality"]
        if not s["error"] and clear and all(cover[k] > 0 for k in need):
            return c, cover
    raise SystemExit(f"{name}: no seed in range covers every case")


def run_reference(GG, cfg):
    draw = CO.InverseCdfDraws(int(cfg["draw_seed"]), int(cfg["B"]))
    RC.pin_multinomial(draw)
    model = GO.StubModel(cfg)
    gen = GG.GraphGenerator(model=model, batch_size=int(cfg["B"]))
    raised, n = -1, -1
    with torch.no_grad():
        try:
            n = gen.build_graphs()
        except IndexError:
            raised = model.calls - 1
    return gen, n, raised, draw


def main():
    assert RC.have_reference()
    blob = {"names": np.array(list(CONFIGS))}
    for name, cfg0 in CONFIGS.items():
        cfg, cover = pick_seeds(name, cfg0)
        with RC.isolated():
            _, GG = RC.load("reference", constants(cfg))
            gen, n, raised, draw = run_reference(GG, cfg)
        s, odraw, _ = GO.run_oracle(cfg)
        if raised >= 0:
            assert s["error"] == GO.ERR_ROUND and s["round"] == raised, (name, raised, s["round"])
        else:
            assert (n, draw.round) == (s["n"], s["round"]), (name, n, draw.round, s["n"], s["round"])
            for k in STATE:
                ref = getattr(gen, k).numpy()
                assert ref.dtype == s[k].dtype and np.array_equal(ref, s[k]), (name, k)
        assert draw.margin == odraw.margin
        for k, v in cfg.items():
            blob[f"{name}::cfg::{k}"] = np.array(v)
        if raised < 0:
            for k in STATE:
                x = getattr(gen, k).numpy()
                blob[f"{name}::{k}"] = x.astype(np.int8) if k in ("nodes", "edges", "generated_nodes",
                                                                  "generated_edges") else x
        blob[f"{name}::n_generated"] = np.array(n)
        blob[f"{name}::rounds"] = np.array(draw.round if raised < 0 else raised)
        blob[f"{name}::raised_round"] = np.array(raised)
        blob[f"{name}::margin"] = np.array(draw.margin)
        print(f"{name}: seeds {cfg['stub_seed']} / {cfg['draw_seed']}, "
              f"{'IndexError at round %d' % raised if raised >= 0 else '%d graphs in %d rounds' % (n, draw.round)}, "
              f"margin {draw.margin:.2e}, coverage {cover}; restatement == unmodified")
    np.savez_compressed(os.path.join(HERE, "golden_grow.npz"), **blob)


if __name__ == "__main__":
    main()
