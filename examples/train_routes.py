"""examples/train_fixture.py fed from MOLECULES instead of preprocessed rows: the whole molecules of the reference's
shipped preprocessed data (the committed .npz conversion of data/pre-training/gdb13_1K-debug/train.h5; the rows
whose f_term entry is set) are the dataset, and their decoding routes are expanded on the device per batch:

    int8 molecules (pinned host memory) -> RouteLoader (gi_reorder.hip: a fresh node order; gi_route.hip: plan, expand,
    merge) -> gnn.mpnn.GGNN(constants) -> apd_kl_loss -> FusedAdam

    python examples/train_routes.py [--epochs 30] [--batch 64] [--model GGNN|AttGGNN] [--no-merge] [--reorder bfs|dfs]

`--reorder` draws a new breadth- or depth-first node order for every molecule in every epoch on the device (route
augmentation: the reference fixes one order per molecule at preprocessing time); without it the molecules are expanded
in the order they are stored in.

A user with only a preprocessed .h5 recovers the molecules the same way (`routes.molecules_from_rows` on the arrays
of `loader.read_hdf_int8`); one with a `PreprocessingGraph` pipeline stores `get_graph_state()` of every molecule
instead of every subgraph."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from examples.train_fixture import constants_for                  # noqa: E402
from graphinvent_amd import dp, routes                            # noqa: E402
from graphinvent_amd.gnn import mpnn                              # noqa: E402
from graphinvent_amd.loss import apd_kl_loss                      # noqa: E402
from graphinvent_amd.optim import FusedAdam                       # noqa: E402


def train(epochs=30, batch=64, model_name="GGNN", merge=True, seed=0, verbose=True, reorder=None, return_model=False):
    d = np.load(os.path.join(ROOT, "tests", "golden", "gdb13_1K-debug_train.npz"))
    nodes, edges = routes.molecules_from_rows(d["nodes"], d["edges"], d["APDs"], unique=True)
    N, Fn = nodes.shape[1:]
    Fe = edges.shape[3]
    dim_f_add, dim_f_conn = [N, 5, Fn - 5, Fe], [N, Fe]            # GDB-13: 5 atom types, then the formal charges
    torch.manual_seed(seed)
    cls = mpnn.GGNN if model_name == "GGNN" else mpnn.AttentionGGNN
    model = cls(constants_for(nodes, edges, d["APDs"])).to("cuda").train()
    opt = FusedAdam(model.parameters(), lr=1e-4)                  # defaults.py:120 init_lr
    loader = routes.RouteLoader(nodes, edges, dim_f_add, dim_f_conn, batch, seed=seed, merge=merge, reorder=reorder)
    steps = 0
    for epoch in range(epochs):                                   # the batch count varies with the epoch's order
        loader.set_epoch(epoch)
        steps += len(loader)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=1e-3, total_steps=steps + 1)
    trainer = dp.DataParallel(model, opt, sched, loss_fn=apd_kl_loss)
    history = []
    for epoch in range(epochs):
        loader.set_epoch(epoch)
        total = torch.zeros((), device="cuda")
        for nb, eb, ab in loader:
            total += trainer.step(nb, eb, ab)
        history.append(float(total) / len(loader))
        if verbose:
            print(f"epoch {epoch:3d}  mean training loss {history[-1]:.4f}")
    if verbose:
        print(f"{nodes.shape[0]} molecules, {int(loader.lengths.sum())} route rows, "
              f"{loader.rows_yielded / epochs:.1f} rows per epoch after the merge")
    return (history, model) if return_model else history


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--model", default="GGNN", choices=["GGNN", "AttGGNN"])
    ap.add_argument("--no-merge", action="store_true")
    ap.add_argument("--reorder", default=None, choices=["bfs", "dfs"])
    a = ap.parse_args()
    train(a.epochs, a.batch, a.model, not a.no_merge, reorder=a.reorder)
