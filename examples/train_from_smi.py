"""examples/train_routes.py fed from a .smi FILE: no preprocessed .h5, no RDKit, no per-molecule Python.

    .smi -> analyze.read_smi (gi_smiles_read.hip: one launch per batch of lines) -> int8 molecules
         -> RouteLoader(reorder="bfs") (gi_reorder.hip, gi_route.hip) -> gnn.mpnn.GGNN -> apd_kl_loss -> FusedAdam

    python examples/train_from_smi.py [--smi FILE] [--epochs 3] [--batch 64] [--reorder bfs|dfs]
                                      [--aromatic error|kekulize] [--atom-types C N O ...] [--max-n-nodes 13]

Without --smi the example writes its own file first: the whole molecules of the reference's shipped preprocessed data
(the committed .npz conversion of gdb13_1K-debug/train.h5) as strings, with `analyze.smiles` and `analyze.write_smi`.

WHAT THE READER IS NOT: no stereo marks and, by default, no aromatic input (c1ccccc1); such lines come back as the empty
molecule with their status bit, are counted and left out here, and belong to RDKit.  With --aromatic kekulize the reader
takes aromatic atoms and assigns the single and double bonds itself (its own rule, not RDKit's kekulisation; a line
without a Kekule structure is left out like any other error).  The atoms of a read molecule are numbered in the
order of the string, NOT in the order the reference's preprocessing would give them — which is why the loader draws a
fresh breadth-first order per molecule and epoch (`reorder="bfs"`), as the reference's routes are breadth-first."""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from examples.train_fixture import constants_for                  # noqa: E402
from graphinvent_amd import analyze, dp, routes                   # noqa: E402
from graphinvent_amd import lib as L                              # noqa: E402
from graphinvent_amd.gnn import mpnn                              # noqa: E402
from graphinvent_amd.loss import apd_kl_loss                      # noqa: E402
from graphinvent_amd.optim import FusedAdam                       # noqa: E402

ATOM_TYPES, FORMAL_CHARGE, MAX_N_NODES = ["C", "N", "O", "S", "Cl"], [-1, 0, 1], 13      # GDB-13's preprocessing_params


def write_fixture_smi(path, rules):
    """The fixture's whole molecules as a .smi file -> the number of lines."""
    d = np.load(os.path.join(ROOT, "tests", "golden", "gdb13_1K-debug_train.npz"))
    nodes, edges = routes.molecules_from_rows(d["nodes"], d["edges"], d["APDs"], unique=True)
    strings = analyze.smiles(torch.from_numpy(nodes).cuda(), torch.from_numpy(edges).cuda(), None, rules)
    analyze.write_smi(path, strings)
    return len(strings)


def train(smi=None, epochs=3, batch=64, seed=0, verbose=True, reorder="bfs", aromatic="error", atom_types=ATOM_TYPES,
          formal_charge=FORMAL_CHARGE, max_n_nodes=MAX_N_NODES):
    rules = analyze.ValenceRules(list(atom_types), list(formal_charge))
    with tempfile.TemporaryDirectory() as tmp:
        if smi is None:
            smi = os.path.join(tmp, "train.smi")
            write_fixture_smi(smi, rules)
        mols = analyze.read_smi(smi, rules, max_n_nodes, aromatic=aromatic)
    keep = (mols.status & L.SMR_READ_ERROR) == 0                  # on the device; the rest goes to RDKit
    nodes, edges = mols.nodes[keep].cpu().numpy(), mols.edges[keep].cpu().numpy()      # the dataset's one read-back
    if verbose:
        left_out = [(k, analyze.describe_read_status(int(s))) for k, s in enumerate(mols.status.tolist()) if s & L.SMR_READ_ERROR]
        print(f"{len(mols)} lines, {len(nodes)} molecules read, {len(left_out)} left out" +
              "".join(f"\n  line {k}: {why}" for k, why in left_out[:5]))
    N, Fn = nodes.shape[1:]
    Fe = edges.shape[3]
    A = len(atom_types)
    dim_f_add, dim_f_conn = [N, A, Fn - A, Fe], [N, Fe]
    apd_shape = np.empty((1, N * A * (Fn - A) * Fe + N * Fe + 1), np.int8)            # shapes only
    torch.manual_seed(seed)
    model = mpnn.GGNN(constants_for(nodes, edges, apd_shape)).to("cuda").train()
    opt = FusedAdam(model.parameters(), lr=1e-4)
    loader = routes.RouteLoader(nodes, edges, dim_f_add, dim_f_conn, batch, seed=seed, reorder=reorder)
    steps = 0
    for epoch in range(epochs):
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
    return history


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--smi", default=None)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reorder", default="bfs", choices=["bfs", "dfs"])
    ap.add_argument("--aromatic", default="error", choices=["error", "kekulize"])
    ap.add_argument("--atom-types", nargs="+", default=ATOM_TYPES)
    ap.add_argument("--formal-charge", nargs="+", type=int, default=FORMAL_CHARGE)
    ap.add_argument("--max-n-nodes", type=int, default=MAX_N_NODES)
    a = ap.parse_args()
    train(a.smi, a.epochs, a.batch, reorder=a.reorder, aromatic=a.aromatic, atom_types=a.atom_types,
          formal_charge=a.formal_charge, max_n_nodes=a.max_n_nodes)
