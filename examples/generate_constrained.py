"""Constrained generation: mask the actions the growth step would reject, or that would break a valence, before the draw.

    python examples/generate_constrained.py [--batch 256] [--epochs 10]

The same model and the same uniforms, with and without ``constraint=``:

    model(nodes, edges) -> [sampler.ActionConstraint -> gi_action_mask (gi_mask.hip)] -> gi_sample_actions -> gi_grow_graphs
                        -> analyze.validity / analyze.fraction_unique                    (gi_valence.hip, gi_canon.hip)

and the fraction valid, properly terminated and unique side by side.  Under the constraint every molecule is valid
and properly terminated by construction.  What that means and what it does not: "valid" is the valence test of THIS
library's table (``analyze.ValenceRules``), not RDKit's sanitisation; the policy sampled is the model's distribution
renormalised over the admissible actions, so ``gen.generated_likelihoods`` are not the unconstrained model's
likelihoods (``likelihood.molecule_log_likelihood`` still scores those).  The model is the GGNN of
examples/train_routes.py after ``--epochs`` epochs on the committed fixture."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from examples.generate_from_scaffolds import Generator            # noqa: E402
from examples.train_routes import train                           # noqa: E402
from graphinvent_amd import analyze                               # noqa: E402
from graphinvent_amd.generator import build_graphs                # noqa: E402
from graphinvent_amd.sampler import ActionConstraint              # noqa: E402

ATOMS, CHARGES = ["C", "N", "O", "F", "S"], [-1, 0, 1]            # hypothetical labels of the fixture's 5 atom types
N, FE = 13, 3


def main(batch=256, epochs=10, seed=0, verbose=True):
    _, model = train(epochs=max(int(epochs), 1), seed=seed, verbose=False, return_model=True)
    model = model.eval()
    groups = [len(ATOMS), len(CHARGES)]
    dim_f_add, dim_f_conn = [N, *groups, FE], [N, FE]
    rules = analyze.ValenceRules(ATOMS, CHARGES, bond_orders=(1, 2, 3))
    constraint = ActionConstraint(rules, dim_f_add, dim_f_conn)
    columns = 2 * (N + N * 6 // 2 - (N - 1) + 1)                   # no constrained run needs more rounds than this
    uniforms = torch.rand(columns, batch, generator=torch.Generator().manual_seed(seed))
    rows = {}
    for name, con in (("unconstrained", None), ("constrained", constraint)):
        gen = Generator(model, batch, N, sum(groups), FE)
        gen.likelihoods = torch.zeros(batch, columns, device="cuda")
        gen.generated_likelihoods = torch.zeros(2 * batch, columns, device="cuda")
        try:
            n = build_graphs(gen, dim_f_add, dim_f_conn, uniforms=uniforms, constraint=con)
        except RuntimeError as e:                                   # the unconstrained model may not finish in time
            n = int((gen.generated_n_nodes != 0).sum())
            if verbose:
                print(f"{name}: {e}")
        mols = gen.generated_nodes[:n], gen.generated_edges[:n], gen.generated_n_nodes[:n]
        v = analyze.validity(*mols, rules, termination=gen.properly_terminated[:n], require_connected=True)
        counts = v.counts.cpu().numpy()
        rows[name] = dict(n=n, rounds=gen.generation_rounds, valid=counts[0] / max(n, 1),
                          terminated=counts[1] / max(n, 1),
                          unique=analyze.fraction_unique(*mols, mask=v.valid) if n else 0.0)
        if con is not None:
            rows[name]["mass_removed_per_graph_round"] = float(
                gen.constraint_stats["mass_removed"] / max(int(gen.constraint_stats["rounds"]) * (batch - 1), 1))
    if verbose:
        print(f"{'':>15} {'molecules':>9} {'rounds':>6} {'valid':>7} {'terminated':>10} {'unique':>7}")
        for name, r in rows.items():
            print(f"{name:>15} {r['n']:>9} {r['rounds']:>6} {r['valid']:>7.3f} {r['terminated']:>10.3f} "
                  f"{r['unique']:>7.3f}")
        print(f"probability mass the mask removed, per graph and round: "
              f"{rows['constrained']['mass_removed_per_graph_round']:.3f}")
    assert rows["constrained"]["valid"] == 1.0 and rows["constrained"]["terminated"] == 1.0
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--epochs", type=int, default=10)
    a = ap.parse_args()
    main(a.batch, a.epochs)
