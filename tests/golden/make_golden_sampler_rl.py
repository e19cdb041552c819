"""Golden vectors for the RL sampling step from the UNMODIFIED reference ``GraphGeneratorRL.get_actions`` /
``get_invalid_actions`` (GraphGeneratorRL.py:521-720) and the reference's autograd through it.

Runs only in the build container (needs /root/reference).  Same set-up as make_golden_sampler.py: stub modules for
rdkit, tqdm, ``parameters.constants`` and ``MolecularGraph``, a bare instance (``object.__new__``) carrying
``batch_size``, ``n_nodes`` and ``edges``, and the one random draw, ``Multinomial(1, probs).sample()``, replaced by a
fixed one-hot (the validity-class fixture of make_golden_sampler.py).  Both APD tensors are
``softmax(logits)`` of leaf logits with ``requires_grad``; the file holds the returned tuples, both likelihoods and
the gradients of ``sum(wa * agent_like) + sum(wp * prior_like)`` with respect to BOTH logits tensors."""
import os
import sys
import types
from collections import namedtuple

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden import make_golden_sampler as MS  # noqa: E402

REF = MS.REF


def load_reference_rl():
    for name in ("rdkit", "tqdm", "MolecularGraph", "parameters", "parameters.constants"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["tqdm"].tqdm = lambda *a, **k: None
    sys.modules["MolecularGraph"].GenerationGraph = object
    sys.modules["parameters.constants"].constants = namedtuple("C", sorted(MS.DIMS))(**MS.DIMS)
    sys.path.insert(0, REF)
    import GraphGeneratorRL
    assert GraphGeneratorRL.__file__.startswith(REF)
    return GraphGeneratorRL


def main():
    GG = load_reference_rl()
    n_nodes, edges, logits, apds, idx = MS.make_inputs()
    B, W = apds.shape
    rng = np.random.default_rng(11)
    prior_logits = (logits + rng.normal(size=logits.shape).astype(np.float32)).astype(np.float32)
    wa = rng.normal(size=B).astype(np.float32)
    wp = rng.normal(size=B).astype(np.float32)
    one_hot = torch.zeros(B, W)
    one_hot[torch.arange(B), torch.from_numpy(idx)] = 1

    class FixedMultinomial:                     # the one random draw, pinned
        def __init__(self, total_count, probs):
            assert total_count == 1 and probs.shape == one_hot.shape

        def sample(self):
            return one_hot.clone()

    torch.distributions.Multinomial = FixedMultinomial
    gen = object.__new__(GG.GraphGeneratorRL)
    gen.batch_size = B
    gen.n_nodes = torch.from_numpy(n_nodes.copy())
    gen.edges = torch.from_numpy(edges.copy())
    la = torch.from_numpy(logits).requires_grad_(True)
    lp = torch.from_numpy(prior_logits).requires_grad_(True)
    softmax = torch.nn.Softmax(dim=1)                                   # GraphGeneratorRL.py:115, 131-132
    add, conn, term, invalid, like_a, like_p = gen.get_actions(agent_apds=softmax(la), prior_apds=softmax(lp))
    (like_a * torch.from_numpy(wa)).sum().add((like_p * torch.from_numpy(wp)).sum()).backward()
    blob = dict(n_nodes=n_nodes, edges=edges.astype(np.int8), agent_logits=logits, prior_logits=prior_logits,
                idx=idx, term=term.numpy(), invalid=invalid.numpy(), agent_likelihoods=like_a.detach().numpy(),
                prior_likelihoods=like_p.detach().numpy(), wa=wa, wp=wp, grad_agent=la.grad.numpy(),
                grad_prior=lp.grad.numpy(), dim_f_add=np.array(MS.DIMS["dim_f_add"]),
                dim_f_conn=np.array(MS.DIMS["dim_f_conn"]))
    for k, t in enumerate(add):
        blob[f"add{k}"] = t.numpy()
    for k, t in enumerate(conn):
        blob[f"conn{k}"] = t.numpy()
    np.savez_compressed(os.path.join(HERE, "golden_sampler_rl.npz"), **blob)
    print("adds", len(add[0]), "conns", len(conn[0]), "terms", len(term), "invalid", len(invalid),
          "|grad_agent|", float(la.grad.abs().max()), "|grad_prior|", float(lp.grad.abs().max()))


if __name__ == "__main__":
    main()
