"""
Model evaluation on the device: the tensor work of ``Analyzer.get_validation_likelihood`` and
``Analyzer.evaluate_model`` (Analyzer.py:39-139, 708-778) that ``Workflow.evaluate_model`` runs every
``sample_every`` epochs.

``get_validation_likelihood(analyzer, dataset, constants)`` is the drop-in for
``analyzer.get_validation_likelihood(dataset)``.  Per batch the reference runs about ten small torch kernels
after the forward (softmax, target normalisation, product, row sum, ``isnan``, ``log``, the slice copy) and a
boolean-mask index whose length depends on the data, i.e. a host synchronisation that drains the queue before
the next forward.  Here the forward is followed by ``gi_eval_nll`` (two launches: one workgroup per row, then
one workgroup that compacts the kept rows into the ``likelihoods`` buffer in row order and counts the
structures), and nothing is read back until the loop is over.

``model_scores(analyzer, likelihood_per_action, constants)`` is ``Analyzer.evaluate_model`` without the file
writes (``util.write_validation_scores`` / ``write_training_status``): the same dictionary, UC-JSD included.
``uc_jsd`` restates the reference's nested ``_uc_jsd`` in torch, quirks and all (``min_len`` over the
zero-padded buffers, ``kl_div`` fed probabilities with its default ``reduction="mean"``, the generated set as
per-action probabilities rather than NLLs).  It runs once per evaluation on a few hundred thousand numbers, so
it has no kernel of its own.
"""
from __future__ import annotations

import torch

from . import lib as L
from .generator import _host_sync_allowed


def action_nll(out: torch.Tensor, target: torch.Tensor, dst: torch.Tensor, start: int,
               n_structures: torch.Tensor, err: torch.Tensor) -> None:
    """One batch of ``get_validation_likelihood`` (Analyzer.py:754-774) in two launches, nothing read back.

    ``out`` [B, W] fp32 logits (any row pitch); ``target`` [B, W] int8 or float (other dtypes are cast to fp32);
    ``dst`` the fp32 ``likelihoods`` buffer: the rows whose correct-action probability is not NaN get their
    NLL at ``dst[start + rank]`` in row order.  ``n_structures`` (fp32, one element) += the sum of
    ``target[:, -1]``.  ``err`` (int32, one element) is set to 1 instead when the kept rows would run past
    ``dst``; the batch then writes and counts nothing, and so does every later call while ``err`` is set."""
    tensors = (out, target, dst, n_structures, err)
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError("action_nll needs CUDA (ROCm) tensors: the MI355X HIP path has no CPU fallback")
    if len({t.device for t in tensors}) != 1:
        raise ValueError("action_nll: all tensors must be on one device")
    if out.dim() != 2 or out.dtype != torch.float32:
        raise TypeError(f"out must be fp32 [B, W], got {out.dtype} {tuple(out.shape)}")
    if target.shape != out.shape:
        raise ValueError(f"target {tuple(target.shape)} does not match out {tuple(out.shape)}")
    if dst.dtype != torch.float32 or dst.dim() != 1 or not dst.is_contiguous():
        raise TypeError("dst must be a contiguous 1-D fp32 tensor")
    if n_structures.dtype != torch.float32 or n_structures.numel() < 1 or not n_structures.is_contiguous():
        raise TypeError("n_structures must be a contiguous fp32 tensor")
    if err.dtype != torch.int32 or err.numel() < 1 or not err.is_contiguous():
        raise TypeError("err must be a contiguous int32 tensor")
    if start < 0:
        raise ValueError("start must be >= 0")
    B, W = out.shape
    if B == 0:                 # the reference adds an empty sum and copies nothing
        return
    if not (out.stride(1) == 1 and out.stride(0) >= W):
        out = out.contiguous()
    if target.dtype == torch.int8:
        tdt = L.DTYPE_I8
    else:
        target, tdt = target.float(), L.DTYPE_F32
    if not (target.stride(1) == 1 and target.stride(0) >= W):
        target = target.contiguous()
    lib = L.load()
    ws = torch.empty(2 * B, dtype=torch.float32, device=out.device)
    with torch.cuda.device(out.device):
        L.check(lib.gi_eval_nll(out.data_ptr(), out.stride(0), target.data_ptr(), tdt, target.stride(0), B, W,
                                dst.data_ptr(), dst.numel(), int(start), n_structures.data_ptr(), err.data_ptr(),
                                ws.data_ptr(), torch.cuda.current_stream(out.device).cuda_stream),
                "gi_eval_nll")


def get_validation_likelihood(analyzer, dataset: str, constants):
    """Drop-in for ``Analyzer.get_validation_likelihood`` (Analyzer.py:708-778): ``analyzer`` is the reference's
    object (duck-typed: ``model``, ``valid_dataloader``, ``train_dataloader``); returns ``(likelihoods,
    avg_final_likelihood)`` as the reference does, with its buffer size, its break test, its placement at
    ``idx * batch_size`` (holes after NaN rows and ragged batches) and its ``ValueError``.

    The loop adds no host synchronisation: with ``model.sync_free = True`` it has none at all.  After the loop
    the overflow word is read once (``RuntimeError`` where the reference's slice assignment would raise) and,
    for a sync-free model, its sticky bounds error (``last_bounded_error``).  The loop runs under
    ``torch.no_grad`` (the reference's caller, ``Workflow.evaluate_model``, does the same)."""
    if dataset == "validation":
        dataloader = analyzer.valid_dataloader
    elif dataset == "training":
        dataloader = analyzer.train_dataloader
    else:
        raise ValueError("Invalid dataset entered.")
    model = analyzer.model
    n_samples = min(100000, constants.n_samples)
    likelihoods = torch.zeros(n_samples * (constants.max_n_nodes + 5), device=constants.device)
    n_structures = torch.zeros(1, device=constants.device)
    if not likelihoods.is_cuda:
        raise RuntimeError("get_validation_likelihood needs constants.device to be a CUDA (ROCm) device: the "
                           "MI355X HIP path has no CPU fallback")
    err = torch.zeros(1, dtype=torch.int32, device=likelihoods.device)
    with torch.no_grad():
        for idx, batch in enumerate(dataloader):
            if idx * constants.batch_size > n_samples:
                break
            if constants.device == "cuda":
                batch = [b.cuda(non_blocking=True) for b in batch]
            nodes, edges, target_output = batch
            action_nll(model(nodes, edges), target_output, likelihoods, idx * constants.batch_size,
                       n_structures, err)
    with _host_sync_allowed():                 # the pass's one read-back, under a caller's sync debug mode
        overflow = int(err.item())
        if getattr(model, "sync_free", False) and hasattr(model, "last_bounded_error"):
            model.last_bounded_error()
    if overflow:
        raise RuntimeError(f"get_validation_likelihood: the {dataset} set's NLLs run past the likelihoods buffer "
                           f"({likelihoods.numel()} entries = n_samples * (max_n_nodes + 5)); the reference's "
                           "slice assignment fails with a shape mismatch here")
    avg_final_likelihood = torch.sum(likelihoods, dim=0) / n_structures[0]
    return likelihoods, avg_final_likelihood


def uc_jsd(likelihood_valid: torch.Tensor, likelihood_train: torch.Tensor,
           likelihood_sampled: torch.Tensor) -> float:
    """``_uc_jsd`` of ``Analyzer.evaluate_model`` (Analyzer.py:49-93), restated in torch."""
    n = min(len(likelihood_valid), len(likelihood_sampled), len(likelihood_train))
    valid = likelihood_valid[:n] / torch.sum(likelihood_valid[:n])
    train = likelihood_train[:n] / torch.sum(likelihood_train[:n])
    sampled = likelihood_sampled[:n] / torch.sum(likelihood_sampled[:n])
    mean = (valid + train + sampled) / 3
    kl = torch.nn.functional.kl_div
    return float((kl(valid, mean) + kl(train, mean) + kl(sampled, mean)) / 3)


def model_scores(analyzer, likelihood_per_action: torch.Tensor, constants) -> dict:
    """``Analyzer.evaluate_model`` (Analyzer.py:39-139) without the writes to ``validation.log`` and the training
    status: the NLL statistics of the validation and training sets (``get_validation_likelihood``), the
    generated set's average and the UC-JSD, under the reference's keys."""
    valid, avg_valid = get_validation_likelihood(analyzer, "validation", constants)
    train, avg_train = get_validation_likelihood(analyzer, "training", constants)
    scores = {
        "likelihood_val": valid,
        "avg_likelihood_val": avg_valid,
        "likelihood_train": train,
        "avg_likelihood_train": avg_train,
        "likelihood_gen": likelihood_per_action,
        "avg_likelihood_gen": torch.sum(likelihood_per_action) / constants.n_samples,
    }
    scores["UC-JSD"] = uc_jsd(scores["likelihood_val"], scores["likelihood_train"], scores["likelihood_gen"])
    return scores
