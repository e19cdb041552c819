"""Test helper: molecule tensors on the device as views INSIDE a larger allocation whose every other element is 1.

The device kernels read a molecule's byte range in 16-byte granules with ragged ends (csrc/gi_molread.h).  A reader that
touches one element outside its range must not find a zero there — zero is the one value that hides it — so the
``misalign`` elements in front of the view and the ``PAD`` elements behind it hold 1: a stray read is a set entry, and
the result differs from the numpy model."""
import numpy as np
import torch

DEV = "cuda"
NP_OF = {torch.float32: np.float32, torch.int8: np.int8}
PAD = 16                                                    # elements behind the view: at least one whole granule


def to_dev(x, dtype=torch.int8, misalign=1):
    """x on the device as `dtype`, contiguous, its first byte `misalign` elements past a 16-byte aligned allocation
    (so that the granules start and end raggedly, and no molecule of a batch sits on a boundary by accident), with
    ones in front of it and behind it."""
    x = np.ascontiguousarray(x)
    buf = torch.ones(misalign + x.size + PAD, dtype=dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[misalign:misalign + x.size].view(x.shape)
    view.copy_(torch.from_numpy(x.astype(NP_OF[dtype])))
    assert view.is_contiguous() and view.storage_offset() == misalign and view._base is buf
    return view


def padding_intact(view) -> bool:
    """Whether everything around a `to_dev` view still holds 1."""
    buf, lo = view._base, view.storage_offset()
    return bool((buf[:lo] == 1).all()) and bool((buf[lo + view.numel():] == 1).all())
