"""Torch restatement of graphinvent_amd.likelihood: rows, molecules, kinds and gradients from logits, ``hot`` and
``row_mol``, on whatever device and dtype the logits have.  No kernel of the library is called here."""
import numpy as np
import torch


def row_ll(logits: torch.Tensor, hot: torch.Tensor) -> torch.Tensor:
    """logits[r, hot[r]] - logsumexp(logits[r]); 0 where hot == -1."""
    hot = hot.long()
    lp = torch.log_softmax(logits, dim=1).gather(1, hot.clamp(min=0)[:, None])[:, 0]
    return torch.where(hot < 0, torch.zeros_like(lp), lp)


def kind_of(hot: torch.Tensor, n_add: int, n_conn: int) -> torch.Tensor:
    """0 add, 1 connect, 2 terminate."""
    hot = hot.long()
    return (hot >= n_add).long() + (hot >= n_add + n_conn).long()


def molecule_ll(rows: torch.Tensor, row_mol: torch.Tensor, M: int) -> torch.Tensor:
    live = row_mol >= 0
    return torch.zeros(M, dtype=rows.dtype, device=rows.device).index_add_(0, row_mol[live].long(), rows[live])


def molecule_kinds(rows: torch.Tensor, hot: torch.Tensor, row_mol: torch.Tensor, M: int, n_add: int,
                   n_conn: int) -> torch.Tensor:
    live = (row_mol >= 0) & (hot >= 0)
    flat = row_mol[live].long() * 3 + kind_of(hot[live], n_add, n_conn)
    return torch.zeros(M * 3, dtype=rows.dtype, device=rows.device).index_add_(0, flat, rows[live]).view(M, 3)


def kind_dims(dim_f_add, dim_f_conn):
    """(n_add, n_conn) of an APD row: f_add.ravel() | f_conn.ravel() | f_term."""
    return int(np.prod(dim_f_add)), int(np.prod(dim_f_conn))


def weighted_objective(logits: torch.Tensor, hot: torch.Tensor, row_mol: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """-(sum_m w_m ll_m) / M, differentiable in the logits."""
    M = w.shape[0]
    return -(w * molecule_ll(row_ll(logits, hot), row_mol, M)).sum() / M


def sequential_sum(rows: np.ndarray, row_mol: np.ndarray, M: int, start=None) -> np.ndarray:
    """The fp32 sum of every molecule's rows, one add per row in row order (what the kernel promises bit for bit)."""
    out = np.zeros(M, np.float32) if start is None else np.array(start, np.float32)
    for v, m in zip(np.asarray(rows, np.float32), row_mol):
        if m >= 0:
            out[m] = np.float32(out[m] + v)
    return out


def sequential_kinds(rows: np.ndarray, hot: np.ndarray, row_mol: np.ndarray, M: int, n_add: int,
                     n_conn: int) -> np.ndarray:
    out = np.zeros((M, 3), np.float32)
    for v, h, m in zip(np.asarray(rows, np.float32), hot, row_mol):
        if m >= 0 and h >= 0:
            k = int(h >= n_add) + int(h >= n_add + n_conn)
            out[m, k] = np.float32(out[m, k] + v)
    return out
