"""Plain-torch restatement of ``Analyzer.get_validation_likelihood`` and the ``_uc_jsd`` nested in
``Analyzer.evaluate_model`` (Analyzer.py:39-139, 708-778), for the tests of graphinvent_amd.evaluate.

The reference checkout is not available on the GPU machine, so the GPU tests compare against this module;
tests/golden/make_golden_eval.py checks it against the unmodified methods bit for bit before it writes
golden_eval.npz, and tests/test_eval_cpu.py does again wherever the reference is visible.

The arithmetic is the reference's, op for op: ``Softmax(dim=1)`` of the logits, the target divided by its row
sum, their product summed over the row, the NaN rows dropped by a boolean mask, ``-1 * log``, the slice
assignment at ``idx * batch_size`` (which raises on a shape mismatch when the buffer is too short), and
``n_structures += sum(target[:, -1])``."""
import torch


def validation_likelihood(model, dataloader, constants, with_count=False):
    """-> (likelihoods, avg_final_likelihood) of ``get_validation_likelihood`` for ``dataloader``
    (``with_count``: and the ``n_structures`` accumulator, which the reference does not return)."""
    n_samples = min(100000, constants.n_samples)
    buf = torch.zeros(n_samples * (constants.max_n_nodes + 5), device=constants.device)
    n_structures = torch.zeros(1, device=constants.device)
    softmax = torch.nn.Softmax(dim=1)
    for idx, batch in enumerate(dataloader):
        if idx * constants.batch_size > n_samples:
            break
        if constants.device == "cuda":
            batch = [b.cuda(non_blocking=True) for b in batch]
        nodes, edges, target = batch
        probs = softmax(model(nodes, edges))
        correct = torch.mul(target / torch.sum(target, dim=1, keepdim=True), probs)
        s = torch.sum(correct, dim=1)
        nll = -1 * torch.log(s[~torch.isnan(s)])
        lo = idx * constants.batch_size
        buf[lo:lo + len(nll)] = nll
        n_structures += torch.sum(target[:, -1]).unsqueeze(dim=0)
    avg = torch.sum(buf, dim=0) / n_structures[0]
    return (buf, avg, n_structures) if with_count else (buf, avg)


def uc_jsd(valid, train, sampled) -> float:
    """``_uc_jsd``: min length over the padded buffers, normalised, ``kl_div(probabilities, mean)``."""
    n = min(len(valid), len(sampled), len(train))
    v = valid[:n] / torch.sum(valid[:n])
    t = train[:n] / torch.sum(train[:n])
    s = sampled[:n] / torch.sum(sampled[:n])
    m = (v + t + s) / 3
    return float((torch.nn.functional.kl_div(v, m) + torch.nn.functional.kl_div(t, m)
                  + torch.nn.functional.kl_div(s, m)) / 3)


def model_scores(model, valid_loader, train_loader, likelihood_per_action, constants) -> dict:
    """The dictionary ``evaluate_model`` hands to ``util.write_validation_scores``."""
    lv, av = validation_likelihood(model, valid_loader, constants)
    lt, at = validation_likelihood(model, train_loader, constants)
    d = {"likelihood_val": lv, "avg_likelihood_val": av, "likelihood_train": lt, "avg_likelihood_train": at,
         "likelihood_gen": likelihood_per_action,
         "avg_likelihood_gen": torch.sum(likelihood_per_action) / constants.n_samples}
    d["UC-JSD"] = uc_jsd(d["likelihood_val"], d["likelihood_train"], d["likelihood_gen"])
    return d


class ListLoader:
    """A plain iterable over fixed batches: row-index lists into (nodes, edges, apds), so that no shuffle can
    change which rows a batch holds.  ``dtype`` None keeps the arrays' own (int8) dtype."""

    def __init__(self, nodes, edges, apds, batches, dtype=torch.float32, device="cpu"):
        self.data = [torch.as_tensor(x) for x in (nodes, edges, apds)]
        self.batches = [list(b) for b in batches]
        self.dtype, self.device = dtype, device

    def __iter__(self):
        for rows in self.batches:
            idx = torch.tensor(rows, dtype=torch.long)
            out = [x[idx] for x in self.data]
            if self.dtype is not None:
                out = [x.to(self.dtype) for x in out]
            yield [x.to(self.device) for x in out]

    def __len__(self):
        return len(self.batches)


class ReplayModel:
    """Returns stored logits batch after batch (the golden's), whatever it is called with."""

    def __init__(self, logits):
        self.logits = list(logits)
        self.calls = 0

    def __call__(self, nodes, edges):
        out = self.logits[self.calls]
        self.calls += 1
        return out
