"""Test helper: the plain torch specification of the graph-level readout glue, the gradient sums behind it and the
optimizer step (csrc/gi_ops.hip through include/graphinvent_amd.h; ``graphinvent_amd.optim.FusedAdam``).  Written from
``oracle/ggnn_oracle.py::graph_gather`` / ``global_readout`` and the header's comments, not from the kernels.  Every
function takes ``dtype``: float64 is the reference, float32 the same formulas in the kernels' own precision — the
yardstick a kernel's error is measured with (tests/test_readout_gpu.py).

Data layout (``check_layout``): a batch of B graphs with N node slots each lives in S compact rows plus the zero row S.
``cidx[b, n]`` is the row of slot n of graph b; every row < S belongs to exactly one slot of the batch, every padded
slot points at row S.  Buffers therefore have S + 1 rows; the functions here take them cut to their payload columns.

  gather_forward   q = fl32(en[cidx] - (mask == 0) * big), att = softmax_n(q), out[b] = sum_n att * emb[cidx]
                   (the one subtraction is formed in fp32 for every dtype: masked energies sit on the 1/16 grid around
                   -1e6 and the kernel performs this subtraction identically; padded slots take part like any slot)
  gather_backward  dg = sum of the given dg; dot = sum_n att * emb * dg; de = att * (emb * dg - dot); dm = att * dg;
                   rows < S: en <- de * dact, emb <- dm * dact; zpart[b] = [sum de | sum dm] over the slots on row S;
                   row S is left alone.  dact = selu' from the stored output, or the factor plane when one is given
  expand           cat[b, n * W + w] = t1[cidx[b, n], w]
  compress         rows < S: t1 <- dcat * dact; zpart[b, w] = sum of dcat over the slots on row S (no dact)
  colsum           out[c] = (sum_r part[r, c]) * selu'(y[c]) (y None: the plain sum)
  slab_sum_dselu   y[r, c] <- selu'(y[r, c]) * sum_s slabs[s, r, c]
  reduce_slabs     dW[n, k] = sum_s slab[s, n, k] (k < K), db[n] = sum_s slab[s, n, K]
  adam_reference   torch.optim.Adam (no amsgrad, L2 weight decay) with the step count kept per GROUP (the deviation
                   documented in graphinvent_amd/optim.py); a parameter without a gradient is skipped entirely"""
import torch

SELU_ALPHA = 1.6732632423543772848170429916717
SELU_SCALE = 1.0507009873554804934193349852946
F64, F32 = torch.float64, torch.float32


def selu_grad_from_out(y, dtype=F64):
    """selu' from the stored output y = selu(z): scale for y > 0, else y + scale * alpha."""
    y = y.to(dtype)
    return torch.where(y > 0, torch.full_like(y, SELU_SCALE), y + torch.tensor(SELU_SCALE * SELU_ALPHA, dtype=dtype))


def check_layout(cidx, S):
    """cidx [B, N] with 0 <= cidx <= S, every compact row < S referenced by exactly one slot of the batch."""
    c = cidx.long().reshape(-1)
    assert cidx.dim() == 2 and int(c.min()) >= 0 and int(c.max()) <= S
    owned = c[c < S]
    assert owned.numel() == S and bool((torch.bincount(owned, minlength=S) == 1).all())
    return c.reshape(cidx.shape)


def batch_layout(N):
    """(cidx, mask, S) of the test batch, int32 [B, N]: graph 0 a single node in slot 0; graph 1 full, no padded slot;
    graph 2 a single node in a middle slot; graph 3 an atom without bonds, its one real row with mask 0, so that every
    slot of the graph is masked; graph 4 real nodes in the first N // 2 slots, the second of them with mask 0.  Only the
    graphs that fit are built: graph 4 needs N >= 4 (B = 4 below that)."""
    rows = [[0], list(range(N)), [N // 2], [0]] + ([list(range(N // 2))] if N >= 4 else [])
    masks = [[1], [1] * N, [1], [0]] + ([[1, 0] + [1] * (N // 2 - 2)] if N >= 4 else [])
    S = sum(len(r) for r in rows)
    cidx = torch.full((len(rows), N), S, dtype=torch.int32)
    mask = torch.zeros((len(rows), N), dtype=torch.int32)
    nxt = 0
    for b, (slots, ms) in enumerate(zip(rows, masks)):
        for n, mk in zip(slots, ms):
            cidx[b, n], mask[b, n] = nxt, mk
            nxt += 1
    check_layout(cidx, S)
    return cidx, mask, S


def masked_energies(en, cidx, mask, big, dtype=F64):
    """[B, N, G]: fl32(en[cidx] - (mask == 0) * big), then converted."""
    pen = (mask == 0).to(F32).unsqueeze(-1) * torch.tensor(big, dtype=F32)
    return (en.to(F32)[cidx.long()] - pen).to(dtype)


def gather_slots(q, embg, dtype=F64):
    """(att, out) from the masked energies q [B, N, G] and the gathered embeddings embg [B, N, G]."""
    att = torch.softmax(q.to(dtype), dim=1)
    return att, torch.sum(att * embg.to(dtype), dim=1)


def gather_slots_backward(q, embg, dg, dtype=F64):
    """(de, dm) per slot [B, N, G] for the upstream gradient dg [B, G]."""
    att, _ = gather_slots(q, embg, dtype)
    d = dg.to(dtype).unsqueeze(1)
    ed = embg.to(dtype) * d
    dot = torch.sum(att * ed, dim=1, keepdim=True)
    return att * (ed - dot), att * d


def gather_forward(en, emb, cidx, mask, big, dtype=F64):
    """out [B, G]; en / emb [S + 1, G], cidx / mask [B, N]."""
    c = check_layout(cidx, en.shape[0] - 1)
    return gather_slots(masked_energies(en, cidx, mask, big, dtype), emb.to(dtype)[c], dtype)[1]


def _scatter_owned(buf, c, S, vals, dact, dtype):
    """rows < S of buf <- vals * dact over the slots that own them; (new buffer, per-graph sums over the others)."""
    new = buf.to(dtype).clone()
    own = c < S
    f = selu_grad_from_out(buf, dtype) if dact is None else dact.to(dtype)
    new[c[own]] = vals[own] * f[c[own]]
    return new, torch.sum(vals * (~own).to(dtype).unsqueeze(-1), dim=1)


def gather_backward(en, emb, cidx, mask, big, S, dg, dact_en=None, dact_emb=None, dtype=F64):
    """(en', emb', zpart [B, 2G]).  dg: a tensor [B, G] or a list of them (summed); dact_*: factor planes [S + 1, G]
    or None for selu' of the stored outputs."""
    assert en.shape[0] == S + 1 == emb.shape[0]
    c = check_layout(cidx, S)
    dgs = [dg] if torch.is_tensor(dg) else [d for d in dg if d is not None]
    d = dgs[0].to(dtype)
    for x in dgs[1:]:
        d = d + x.to(dtype)
    de, dm = gather_slots_backward(masked_energies(en, cidx, mask, big, dtype), emb.to(dtype)[c], d, dtype)
    en_new, zen = _scatter_owned(en, c, S, de, dact_en, dtype)
    emb_new, zemb = _scatter_owned(emb, c, S, dm, dact_emb, dtype)
    return en_new, emb_new, torch.cat((zen, zemb), dim=1)


def expand(t1, cidx, dtype=None):
    """cat [B, N * W]: a copy, in t1's dtype unless one is given."""
    c = check_layout(cidx, t1.shape[0] - 1)
    t = t1 if dtype is None else t1.to(dtype)
    return t[c].reshape(c.shape[0], -1)


def compress(t1, cidx, S, dcat, dact=None, dtype=F64):
    """(t1', zpart [B, W]); dcat [B, N * W]."""
    assert t1.shape[0] == S + 1
    c = check_layout(cidx, S)
    B, N = c.shape
    return _scatter_owned(t1, c, S, dcat.to(dtype).reshape(B, N, -1), dact, dtype)


def colsum(part, y=None, dtype=F64):
    s = part.to(dtype).sum(dim=0)
    return s if y is None else s * selu_grad_from_out(y, dtype)


def slab_sum_dselu(slabs, y, dtype=F64):
    """slabs [nsplit, rows, cols], y [rows, cols] the stored outputs."""
    return slabs.to(dtype).sum(dim=0) * selu_grad_from_out(y, dtype)


def reduce_slabs(slabs, dtype=F64):
    """slabs [n_slabs, N, K + 1] -> (dW [N, K], db [N])."""
    s = slabs.to(dtype).sum(dim=0)
    return s[:, :-1], s[:, -1]


def adam_reference(params, groups, grads, betas=(0.9, 0.999), eps=1e-8, dtype=F64):
    """params: list of tensors; groups: list of dict(idx=[parameter numbers], lr, weight_decay); grads: one list per
    step holding a tensor or None per parameter.  Returns one (params, exp_avg, exp_avg_sq) snapshot per step."""
    p = [x.detach().to(dtype).clone() for x in params]
    m = [torch.zeros_like(x) for x in p]
    v = [torch.zeros_like(x) for x in p]
    count = [0] * len(groups)
    b1, b2 = betas
    history = []
    for step_grads in grads:
        for gi, grp in enumerate(groups):
            if all(step_grads[i] is None for i in grp["idx"]):
                continue
            count[gi] += 1
            t = count[gi]
            step_size = grp["lr"] / (1.0 - b1 ** t)
            bc2_sqrt = (1.0 - b2 ** t) ** 0.5
            for i in grp["idx"]:
                if step_grads[i] is None:
                    continue
                g = step_grads[i].to(dtype) + grp["weight_decay"] * p[i]
                m[i] = m[i] + (1.0 - b1) * (g - m[i])
                v[i] = b2 * v[i] + (1.0 - b2) * g * g
                p[i] = p[i] - step_size * (m[i] / (v[i].sqrt() / bc2_sqrt + eps))
        history.append(([x.clone() for x in p], [x.clone() for x in m], [x.clone() for x in v]))
    return history
