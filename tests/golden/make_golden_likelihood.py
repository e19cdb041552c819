"""Golden log-likelihoods of whole molecules, produced in the build container from the UNMODIFIED reference:
``gnn.mpnn.GGNN`` on the CPU with the trained small-model weights of golden_generator.npz (``w::*``, H = 32), and
``Analyzer.get_validation_likelihood`` (Analyzer.py:708-778) for the per-row expression.

Data: the ``gdb13::`` set of golden_routes.npz — 140 molecules, 1360 route rows, route lengths 2 to 18, W = 625; its
``rows_nodes`` / ``rows_edges`` / ``hot`` / ``row_mol`` are the reference's ``get_decoding_route_state`` already.

Stored (reference logits are NOT stored: the tests recompute them with oracle/ggnn_oracle.py):

* ``row_ll_ref32``   per row, the reference's own fp32 expression: ``-1 *`` what the unmodified
  ``get_validation_likelihood`` leaves in its ``likelihoods`` buffer for one-hot targets (softmax, t / T * p, row
  sum, log), the rows fed in order in batches of 200
* ``row_ll``         per row, fp64 in log space on the same logits: ``z[hot] - logsumexp(z)``
* ``mol_ll`` / ``mol_kind``   per molecule, the fp64 sums of ``row_ll`` and their split into add / connect / terminate
* ``w_seed`` / ``w``  the molecule weights (``default_rng(w_seed).uniform(0.5, 1.5, M)`` as fp32), and ``g::<name>``:
  every parameter's fp32 gradient of ``-(sum_m w_m ll_m) / M``, ll in fp32 through ``log_softmax`` on the reference
  model's tape (all rows in one batch)
* ``logit_absmax``, ``chunk_shift`` (how far the reference's own logits move, absolute, when the same rows are fed in
  chunks of 37 instead of 200) and ``f32_vs_f64`` (max |row_ll_ref32 - row_ll| / max |row_ll|)

Checked here with the reference alone: every row value is finite; row ``ll`` within [-44.3, -9e-7] and molecule ``ll``
within [-422.5, -1.77]; ``f32_vs_f64`` <= 2e-7; ``chunk_shift`` <= 2e-5.

Run from the repository root: ``python tests/golden/make_golden_likelihood.py``."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ggnn_oracle as O                # noqa: E402
from tests import eval_oracle as EO                # noqa: E402
from tests import likelihood_model as LM           # noqa: E402
from tests.golden import make_golden_eval as MGE   # noqa: E402
from tests.golden import ref_callers as RC         # noqa: E402

W_SEED = 20241018
SET = "gdb13::"


def chunked(model, nodes, edges, size):
    with torch.no_grad():
        return torch.cat([model(nodes[i:i + size], edges[i:i + size]) for i in range(0, nodes.shape[0], size)])


def main():
    assert RC.have_reference()
    G = np.load(os.path.join(HERE, "golden_generator.npz"))
    Rt = np.load(os.path.join(HERE, "golden_routes.npz"))
    cfg = O.make_config(**{str(k): int(v) for k, v in zip(G["cfg_keys"], G["cfg_vals"])})
    rows_n, rows_e = Rt[SET + "rows_nodes"], Rt[SET + "rows_edges"]
    hot, row_mol = Rt[SET + "hot"].astype(np.int64), Rt[SET + "row_mol"].astype(np.int64)
    dim_f_add, dim_f_conn = Rt[SET + "dim_f_add"], Rt[SET + "dim_f_conn"]
    R, M, W = rows_n.shape[0], int(row_mol.max()) + 1, O.apd_width(cfg)
    n_add, n_conn = LM.kind_dims(dim_f_add, dim_f_conn)
    assert (R, M, W) == (1360, 140, 625) and n_add + n_conn + 1 == W
    lengths = np.bincount(row_mol, minlength=M)
    assert lengths.min() == 2 and lengths.max() == 18

    bs = 200
    consts = MGE.consts_for(cfg, bs, R + bs)                    # the break test never fires before the last batch
    AN, mpnn, _ = MGE.load_reference(consts)
    model = mpnn.GGNN(consts)
    model.load_state_dict({k[3:]: torch.from_numpy(G[k]) for k in G.files if k.startswith("w::")})
    model.eval()

    # ---- rows: the unmodified get_validation_likelihood on one-hot targets ------------------------------
    apds = np.zeros((R, W), np.int8)
    apds[np.arange(R), hot] = 1
    batches = [range(i, min(i + bs, R)) for i in range(0, R, bs)]
    AN.constants = consts
    a = AN.Analyzer.__new__(AN.Analyzer)
    a.model = MGE.Recorder(model)
    a.valid_dataloader = a.train_dataloader = EO.ListLoader(rows_n, rows_e, apds, batches)
    with torch.no_grad():
        like, _ = a.get_validation_likelihood(dataset="validation")
    assert len(a.model.logits) == len(batches)
    nll32 = torch.cat([like[i * bs:i * bs + len(b)] for i, b in enumerate(batches)])
    assert int((like != 0).sum()) == R == nll32.numel()
    z = torch.cat(a.model.logits)
    row32 = (-nll32).numpy()
    row64 = LM.row_ll(z.double(), torch.from_numpy(hot)).numpy()
    assert np.isfinite(row32).all() and np.isfinite(row64).all()
    mol64 = LM.molecule_ll(torch.from_numpy(row64), torch.from_numpy(row_mol), M).numpy()
    kind64 = LM.molecule_kinds(torch.from_numpy(row64), torch.from_numpy(hot), torch.from_numpy(row_mol), M, n_add,
                               n_conn).numpy()
    assert np.abs(kind64.sum(1) - mol64).max() < 1e-9
    f32_vs_f64 = float(np.abs(row32 - row64).max() / np.abs(row64).max())
    nodes_f, edges_f = torch.from_numpy(rows_n).float(), torch.from_numpy(rows_e).float()
    assert torch.equal(chunked(model, nodes_f, edges_f, bs), z)
    chunk_shift = float((chunked(model, nodes_f, edges_f, 37) - z).abs().max())
    print(f"rows {R}: ll in [{row64.min():.4g}, {row64.max():.4g}]; molecules {M}: ll in [{mol64.min():.4g}, "
          f"{mol64.max():.4g}]; fp32 vs fp64 {f32_vs_f64:.2e}; max |logit| {float(z.abs().max()):.4g}; "
          f"chunks of 37 move the logits by {chunk_shift:.2e}")
    assert -44.3 <= row64.min() and row64.max() <= -9e-7
    assert -422.5 <= mol64.min() and mol64.max() <= -1.77
    assert f32_vs_f64 <= 2e-7 and chunk_shift <= 2e-5

    # ---- gradients ---------------------------------------------------------------------------------------
    w = np.random.default_rng(W_SEED).uniform(0.5, 1.5, M).astype(np.float32)
    model.zero_grad()
    loss = LM.weighted_objective(model(nodes_f, edges_f), torch.from_numpy(hot), torch.from_numpy(row_mol),
                                 torch.from_numpy(w))
    loss.backward()
    ref_loss = -float((w.astype(np.float64) * mol64).sum() / M)
    assert abs(float(loss.detach()) - ref_loss) <= 1e-5 * abs(ref_loss), (float(loss.detach()), ref_loss)
    blob = dict(cfg_keys=G["cfg_keys"], cfg_vals=G["cfg_vals"], set=np.array(SET), row_ll_ref32=row32, row_ll=row64,
                mol_ll=mol64, mol_kind=kind64, w_seed=np.int64(W_SEED), w=w, loss=np.float64(float(loss.detach())),
                logit_absmax=np.float64(float(z.abs().max())), chunk_shift=np.float64(chunk_shift),
                f32_vs_f64=np.float64(f32_vs_f64))
    for k, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        blob["g::" + k] = p.grad.numpy().copy()
    out = os.path.join(HERE, "golden_likelihood.npz")
    np.savez_compressed(out, **blob)
    print(out, os.path.getsize(out), "bytes; loss", float(loss.detach()))


if __name__ == "__main__":
    with RC.isolated():
        main()
