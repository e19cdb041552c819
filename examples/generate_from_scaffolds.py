"""Seeded generation: grow molecules from given scaffolds instead of from the empty graph.

    python examples/generate_from_scaffolds.py [--seeds 4] [--atoms 4] [--batch 32] [--epochs 10]

A few molecules of the reference's shipped preprocessed data (the committed .npz conversion of
data/pre-training/gdb13_1K-debug/train.h5, through `routes.molecules_from_rows`) are truncated to their first k atoms
— a prefix of a molecule in decoding order is itself a molecule in decoding order — and become the seed bank:

    int8 molecules -> generator.SeedBank (validated once on the device, gi_route.hip)
                   -> generator.build_graphs(gen, dim_f_add, dim_f_conn, seeds=bank)    (gi_grow.hip)
                   -> analyze.decode (gi_analyze.hip) -> seed and product side by side

Every graph of the batch starts from a seed and restarts from the next one when it is written out, round-robin over
the bank; `gen.generated_seed` names the seed behind every generated molecule.  The model is the GGNN of
examples/train_routes.py after `--epochs` epochs on the same fixture (a few seconds; an untrained model ends almost
every graph at once through an invalid action)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from examples.train_routes import train                           # noqa: E402
from graphinvent_amd import analyze, routes                       # noqa: E402
from graphinvent_amd.generator import SeedBank, build_graphs      # noqa: E402

ATOMS = "CNOFS"                                                   # hypothetical labels of the fixture's 5 atom types


class Generator:
    """The fields of the reference's GraphGenerator after __init__ (GraphGenerator.py:27-43)."""

    def __init__(self, model, B, N, Fn, Fe):
        z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device="cuda")
        self.model, self.batch_size = model, B
        self.nodes, self.edges, self.n_nodes = z(B, N, Fn), z(B, N, N, Fe), z(B, dtype=torch.int8)
        self.nodes[0], self.edges[0, 0, 0, 0], self.n_nodes[0] = 1, 1, 1          # the dummy graph
        self.likelihoods, self.generated_likelihoods = z(B, 2 * N), z(2 * B, 2 * N)
        self.generated_nodes, self.generated_edges = z(2 * B, N, Fn), z(2 * B, N, N, Fe)
        self.generated_n_nodes, self.properly_terminated = z(2 * B, dtype=torch.int8), z(2 * B, dtype=torch.int8)


def formula(atoms, bonds):
    """A one-line description of a decoded molecule: its atoms and its bonds (i-j:type)."""
    a = "".join(ATOMS[t] if 0 <= t < len(ATOMS) else "?" for t in atoms[:, 0])
    return f"{a or '(empty)':<14} " + " ".join(f"{i}-{j}:{t}" for i, j, t in bonds)


def main(n_seeds=4, k=4, batch=32, epochs=10, seed=0, verbose=True):
    d = np.load(os.path.join(ROOT, "tests", "golden", "gdb13_1K-debug_train.npz"))
    nodes, edges = routes.molecules_from_rows(d["nodes"], d["edges"], d["APDs"], unique=True)
    N, Fn = nodes.shape[1:]
    Fe = edges.shape[3]
    groups = [5, Fn - 5]
    dim_f_add, dim_f_conn = [N, *groups, Fe], [N, Fe]
    # the seeds: the first k atoms of a few molecules, with the bonds among them
    big = np.flatnonzero(nodes.any(axis=2).sum(axis=1) > k)[:n_seeds]
    seed_nodes, seed_edges = nodes[big].copy(), edges[big].copy()
    seed_nodes[:, k:] = 0
    seed_edges[:, k:] = 0
    seed_edges[:, :, k:] = 0
    bank = SeedBank(torch.from_numpy(seed_nodes).cuda(), torch.from_numpy(seed_edges).cuda(), dim_f_add, dim_f_conn)

    _, model = train(epochs=max(int(epochs), 1), seed=seed, verbose=False, return_model=True)
    model = model.eval()
    gen = Generator(model, batch, N, Fn, Fe)
    n = build_graphs(gen, dim_f_add, dim_f_conn, generator=torch.Generator(device="cuda").manual_seed(seed),
                     seeds=bank)
    seeds_dec = analyze.decode(bank.nodes, bank.edges, bank.n_nodes, groups)
    out_dec = analyze.decode(gen.generated_nodes[:n], gen.generated_edges[:n], gen.generated_n_nodes[:n], groups)
    which = gen.generated_seed[:n].cpu().numpy()
    rows = []
    for i in range(n):
        sa, sb, _ = seeds_dec.molecule(int(which[i]))
        pa, pb, _ = out_dec.molecule(i)
        rows.append((int(which[i]), formula(sa, sb), formula(pa, pb)))
        assert len(pa) >= len(sa) and (pa[:len(sa)] == sa).all()      # the product contains its seed
    if verbose:
        print(f"{n} molecules from {len(bank)} seeds of {k} atoms in {gen.generation_rounds} rounds")
        grown = sum(a != b for _, a, b in rows)
        print(f"{grown} of them grew beyond their seed; the first few:")
        for s, a, b in sorted(rows, key=lambda r: r[1] == r[2])[:12]:
            print(f"seed {s}: {a}\n     -> {b}")
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=4)
    ap.add_argument("--atoms", type=int, default=4)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--epochs", type=int, default=10)
    a = ap.parse_args()
    main(a.seeds, a.atoms, a.batch, a.epochs)
