"""
Read-out of generated molecules on the device: the tensor bookkeeping of ``Analyzer.get_molecular_properties``
(Analyzer.py:311-599) and of ``GraphGenerator.graph_to_graph`` / ``GraphGeneratorRL.graph_to_graph``
(GraphGenerator.py:659-804, GraphGeneratorRL.py:725-), which the reference does molecule by molecule from Python:
``int(torch.sum(edges[node, :, bond]))`` for every molecule, node and bond type, a ``torch.nonzero`` per node and per
graph and ``.item()`` on every bond index, i.e. one device-to-host synchronisation per atom and per bond.

``molecular_properties(nodes, edges, n_nodes, groups, ...)`` is one launch (``gi_mol_properties``) over the generator's
own tensors and returns the dictionary entries of ``get_molecular_properties`` that need no RDKit, as fp32 tensors on
the device with the reference's shapes and values.  ``fraction_valid`` and ``fraction_valid_properly_terminated`` are
NOT produced by that call: the caller merges them into the dictionary from ``fraction_valid`` below (or from RDKit's
sanitisation), as it does ``fraction_unique`` (from ``fraction_unique`` below, with the validity as the mask).

``ValenceRules`` / ``validity`` / ``fraction_valid`` decide which molecules are VALID, on the device
(``gi_mol_valence``): the reference's ``validity_tensor`` (util.py:549-585, one ``SanitizeMol`` per molecule) as a
valence test of the labelled graph — a table look-up per atom, NOT RDKit's sanitisation, no kekulisation — together
with the hydrogen fill, mass, component and ring counts of every molecule, see ``validity``.

``canonical`` / ``unique`` / ``fraction_unique`` / ``SeenSet`` decide which molecules are the SAME molecule, on the
device (``gi_mol_canon``, ``gi_mol_unique``, ``gi_mol_seen_add``): the reference's ``uniqueness_tensor``
(util.py:549-585) and ``fraction_unique`` (Analyzer.py:480-499) without a SMILES string.  Identity here is isomorphism
of the labelled graph (node feature rows, bond types), see ``canonical``.

``fingerprint`` / ``FingerprintSet`` / ``similarity`` / ``KernelModel`` / ``activity`` / ``internal_diversity`` SCORE
molecules on the device (``gi_mol_fingerprint``, ``gi_fp_compare``): the reference's ``"activity"`` score component
(ScoringFunction.py:145-192, one RDKit Morgan fingerprint and one scikit-learn ``predict_proba`` per molecule on the
host) over a Morgan-style fingerprint of the labelled graph — NOT RDKit's ECFP bits, see ``fingerprint`` — and
nearest-neighbour similarity to a stored set; ``target_size_score`` / ``compute_score`` restate the rest of
``ScoringFunction.compute_score`` in plain torch.

``decode(nodes, edges, n_nodes, groups)`` is one launch (``gi_mol_decode``) that writes what ``_graph_to_mol`` reads
out of the tensors: per atom the index inside each one-hot segment, per graph the bond triples in
``torch.nonzero``'s order, and a status word for what the reference would misread or raise on.  ``.host()`` brings all
of it to the host with one copy and one synchronisation; ``records`` maps the indices through the constants' tables
into the arguments of ``Chem.Atom`` / ``AddBond``.  Building ``rdkit.Chem.RWMol`` objects stays in the caller.

``smiles`` / ``write_smi`` write the molecules as SMILES strings on the device (``gi_mol_smiles``) and as a ``.smi``
file: the product of the reference's ``util.write_graphs_to_smi``.  The string is a faithful spelling of the labelled
graph in an OpenSMILES subset — NOT RDKit's canonical SMILES: no aromaticity, no stereo, see ``smiles``.

``pack_strings`` / ``read_smiles`` / ``read_smi`` go the other way (``gi_smiles_read``): SMILES strings and ``.smi``
files into the int8 molecules that ``routes.RouteLoader``, ``SeedBank``, ``SeenSet`` and ``FingerprintSet`` take — the
reference's RDKit preprocessing on the writer's subset: no stereo, atoms in string order, aromatic input only with
``aromatic="kekulize"`` (``gi_smiles_read_arom``) and then kekulised by the library's own rule, not RDKit's, see
``read_smiles``.

``resonance`` / ``kekulize`` / ``canonical_compound`` give ONE IDENTITY PER COMPOUND (``gi_mol_resonance``,
``gi_mol_kekulize``): which bonds change order between the Kekule structures of a molecule, the molecule with those
bonds in a channel of their own (the normal form ``canonical`` / ``unique`` / ``SeenSet`` then compare) and back to one
canonical Kekule structure — a definition without chemistry tables, NOT aromaticity perception, see ``resonance``.

Counts are summed as integers on the device and converted once (the exact integer as fp32, then one fp32 division):
bit for bit the reference's values while every count is below 2**24.  Beyond that the reference's own fp32
accumulation (``hist[i] += 1``) stops being exact, e.g. it stays at 16777216 for ever; the counts here stay exact
integers (rounded once to fp32), which is deliberately not the reference's result.
"""
from __future__ import annotations

import ctypes as C
import functools
import math
from typing import Iterator, Optional, Sequence

import numpy as np
import torch

from . import lib as L
from .generator import _host_sync_allowed

#: status bits of ``decode`` (``lib.MOL_*``), with what the reference does in that case
STATUS_MESSAGES = {
    L.MOL_ONEHOT: "a node row below n_nodes does not have exactly one set entry per segment (the reference reads "
                  "the wrong entries or raises IndexError)",
    L.MOL_BOND_PAST_N: "a bond touches a node >= n_nodes (the reference raises KeyError in node_to_idx)",
    L.MOL_OVERFLOW: "more than max_bonds bonds (only the first max_bonds are written; n_bonds holds the true count)",
    L.MOL_VALUE: "an entry is neither 0 nor 1",
    L.MOL_MULTI_BOND: "a pair of atoms carries several bond types (RDKit's AddBond refuses the second)",
}


def describe_status(bits: int) -> str:
    return "; ".join(msg for bit, msg in STATUS_MESSAGES.items() if bits & bit) or "well-formed"


def _check_inputs(what: str, nodes, edges, n_nodes, groups: Sequence[int], need_n_nodes: bool):
    """-> (G, N, Fn, Fe, dtype code, n_nodes (or None), its byte width, groups as ints)."""
    for name, x in (("nodes", nodes), ("edges", edges)):
        if not isinstance(x, torch.Tensor):
            raise TypeError(f"{what}: {name} must be a torch tensor, got {type(x).__name__}")
        if not x.is_cuda:
            raise RuntimeError(f"{what} needs CUDA (ROCm) tensors ({name} is on {x.device}): the MI355X HIP path has "
                               "no CPU fallback")
    if nodes.dim() != 3 or edges.dim() != 4:
        raise ValueError(f"{what}: nodes must be [G, N, Fn] and edges [G, N, N, Fe]")
    G, N, Fn = nodes.shape
    Fe = edges.shape[3]
    if tuple(edges.shape) != (G, N, N, Fe):
        raise ValueError(f"{what}: edges {tuple(edges.shape)} does not match nodes {tuple(nodes.shape)}")
    if nodes.dtype != edges.dtype or nodes.dtype not in (torch.float32, torch.int8):
        raise TypeError(f"{what}: nodes and edges must both be float32 or both int8, got {nodes.dtype} / {edges.dtype}")
    if edges.device != nodes.device:
        raise ValueError(f"{what}: edges is on {edges.device}, nodes on {nodes.device}")
    if not nodes.is_contiguous() or not edges.is_contiguous():
        raise ValueError(f"{what}: nodes and edges must be contiguous (they are read in place, once)")
    groups = None if groups is None else [int(g) for g in groups]     # None: the caller has no use for segments
    if groups is not None and (not 2 <= len(groups) <= 4 or min(groups) < 1 or sum(groups) != Fn):
        raise ValueError(f"{what}: groups {groups} must be 2 to 4 positive segment sizes (atom type, formal charge, "
                         f"[implicit H], [chirality]) that sum to Fn = {Fn}")
    if N < 1 or Fn < 1 or Fe < 1 or N > L.GI_MAX_NODES or Fe > L.GI_MAX_GROUPS or Fn > L.ANALYZE_MAX_FN:
        raise ValueError(f"{what}: needs 1 <= N <= {L.GI_MAX_NODES}, 1 <= Fe <= {L.GI_MAX_GROUPS}, 1 <= Fn <= "
                         f"{L.ANALYZE_MAX_FN}; got N {N}, Fn {Fn}, Fe {Fe}")
    nn_bytes = 1
    if n_nodes is None:
        if need_n_nodes:
            raise ValueError(f"{what}: n_nodes is required")
    else:
        if not isinstance(n_nodes, torch.Tensor):
            raise TypeError(f"{what}: n_nodes must be a torch tensor")
        if not n_nodes.is_cuda or n_nodes.device != nodes.device:
            raise RuntimeError(f"{what}: n_nodes must be a CUDA tensor on {nodes.device} (no CPU fallback)")
        if tuple(n_nodes.shape) != (G,):
            raise ValueError(f"{what}: n_nodes has shape {tuple(n_nodes.shape)}, expected ({G},)")
        if n_nodes.dtype not in (torch.int8, torch.int32, torch.int64):
            raise TypeError(f"{what}: n_nodes must be int8 (what build_graphs leaves), int32 or int64, got "
                            f"{n_nodes.dtype}")
        if not n_nodes.is_contiguous():
            raise ValueError(f"{what}: n_nodes must be contiguous")
        nn_bytes = n_nodes.element_size()
    dtype = L.DTYPE_I8 if nodes.dtype == torch.int8 else L.DTYPE_F32
    return G, N, Fn, Fe, dtype, n_nodes, nn_bytes, groups


def _check_termination(what: str, termination, G: int, dev):
    """-> (termination as contiguous int8 or fp32 (or None), its dtype code)."""
    if termination is None:
        return None, L.DTYPE_I8
    if not isinstance(termination, torch.Tensor) or not termination.is_cuda or termination.device != dev:
        raise RuntimeError(f"{what}: termination must be a CUDA tensor on {dev} (no CPU fallback)")
    if tuple(termination.shape) != (G,):
        raise ValueError(f"{what}: termination has shape {tuple(termination.shape)}, expected ({G},)")
    if termination.dtype == torch.int8:
        return termination.contiguous(), L.DTYPE_I8
    return termination.float().contiguous(), L.DTYPE_F32


_ITEMSIZE = {"int8": 1, "uint8": 1, "int16": 2, "int32": 4, "int64": 8, "float32": 4}


def _pack(*arrays) -> dict:
    """``(name, dtype name, shape), ...`` in byte order -> ``name -> (byte offset, bytes, dtype name, shape)``."""
    table, off = {}, 0
    for name, dtype, shape in arrays:
        item = _ITEMSIZE[dtype]
        assert off % item == 0, name                        # every array is aligned to its element size
        table[name] = (off, item * math.prod(shape), dtype, shape)
        off += table[name][1]
    return table


class _ResultBuffer:
    """The outputs of one launch as arrays inside ONE byte buffer on the device, so that ``host()`` needs one copy.
    A subclass declares ``layout(*dims)`` (a ``_pack`` table, kept per dims: a launch-bound call cannot afford to
    rebuild it) and what ``host()`` returns (``_host_result``).  The device views are attributes made when first
    asked for (a caller that wants one does not pay for all, and the launch takes its pointers from ``_ptrs()``,
    without a view); ``_HOST_DTYPE`` names the arrays whose numpy dtype differs from the device's."""

    _HOST_DTYPE: dict = {}

    def __init__(self, buf: torch.Tensor, G: int, *dims: int):
        self._buf, self._layout, self._host, self._pinned = buf, self.layout(G, *dims), None, None
        self.G = G

    @classmethod
    def nbytes(cls, *dims: int) -> int:
        off, size, _, _ = next(reversed(cls.layout(*dims).values()))          # the last array ends the buffer
        return off + size

    @classmethod
    def empty(cls, dev, *dims: int, **kw):
        return cls(torch.empty(cls.nbytes(*dims), dtype=torch.uint8, device=dev), *dims, **kw)

    def _ptrs(self) -> dict:
        base = self._buf.data_ptr()
        return {name: base + entry[0] for name, entry in self._layout.items()}

    def _view(self, name, buf, xp):
        off, size, dtype, shape = self._layout[name]
        if xp is np:
            dtype = self._HOST_DTYPE.get(name, dtype)
        return buf[off:off + size].view(getattr(xp, dtype)).reshape(shape)

    def __getattr__(self, name):
        if name in self.__dict__.get("_layout", ()):
            view = self.__dict__[name] = self._view(name, self._buf, torch)
            return view
        raise AttributeError(name)

    def host(self):
        """All arrays as numpy arrays on the host: ONE asynchronous copy of the buffer into pinned memory and ONE
        synchronisation (of the current stream), done once and kept."""
        if self._host is None:
            dev = self._buf.device
            with _host_sync_allowed():                  # the read-out's one wait, under a caller's sync debug mode
                pinned = torch.empty(self._buf.numel(), dtype=torch.uint8, pin_memory=True)
                if pinned.numel() > 0:
                    stream = torch.cuda.current_stream(dev)
                    with torch.cuda.device(dev):
                        pinned.copy_(self._buf, non_blocking=True)
                    stream.synchronize()
            self._pinned = pinned                       # the arrays are views of it
            host = pinned.numpy()
            self._host = self._host_result({name: self._view(name, host, np) for name in self._layout})
        return self._host

    def __len__(self):
        return self.G


def molecular_properties(nodes: torch.Tensor, edges: torch.Tensor, n_nodes: Optional[torch.Tensor],
                         groups: Sequence[int], *, termination: Optional[torch.Tensor] = None,
                         epoch_key: Optional[str] = None, max_n_nodes: Optional[int] = None,
                         n_imp_H: int = 0, n_chirality: int = 0, use_imp_H: Optional[bool] = None,
                         use_chirality: Optional[bool] = None) -> dict:
    """The entries of ``Analyzer.get_molecular_properties`` (Analyzer.py:311-599) that need no RDKit, in one launch.

    ``nodes`` [G, N, Fn] / ``edges`` [G, N, N, Fe]: contiguous device tensors, both fp32 or both int8 (e.g. a
    generator's ``generated_nodes`` / ``generated_edges``, or the int8 molecule arrays of ``routes.RouteLoader`` for
    ``evaluate_training_set``).  ``n_nodes`` [G] int8 / int32 / int64; ``None`` derives it as the number of non-zero
    node rows (the model's node mask).  ``groups``: the sizes of the one-hot segments of a node row in the
    reference's order — atom type, formal charge, [implicit H], [chirality] — i.e. the differences of
    ``util.get_feature_vector_indices()``.  With three groups, ``use_imp_H`` / ``use_chirality`` say which optional
    segment the third one is (default: implicit H unless ``use_chirality`` is set alone).  An absent segment is the
    reference's ``[0] * n`` list of length ``n_imp_H`` / ``n_chirality``.  ``max_n_nodes`` (default N) sizes
    ``n_nodes_hist``.  ``termination`` [G] (int8 or float) adds ``fraction_properly_terminated``.

    Returns ``{name: value}``, or ``{(epoch_key, name): value}`` when ``epoch_key`` is given, for ``n_nodes_hist``
    [max_n_nodes + 1], ``avg_n_nodes``, ``atom_type_hist``, ``formal_charge_hist``, ``numh_hist``,
    ``chirality_hist``, ``n_edges_hist`` [10], ``avg_n_edges``, ``edge_feature_hist`` [Fe] and (with
    ``termination``) ``fraction_properly_terminated``: fp32 tensors on the device (views of one buffer), quirks
    included — a node of degree 0 is counted in the LAST bin of ``n_edges_hist``, the column sums run over all N
    rows, ``edge_feature_hist`` halves the whole plane's sum.  Nothing is read back and nothing synchronises.

    NOT produced: ``fraction_unique``, ``fraction_valid``, ``fraction_valid_properly_terminated``.  They come from
    ``fraction_unique`` and ``fraction_valid`` of this module (or from RDKit); merge them into the dictionary in the
    caller.  Values are the reference's bit for bit while every count
    is below 2**24 (see the module docstring for what happens beyond).  G = 0 returns zeros without a launch (the
    reference raises)."""
    what = "molecular_properties"
    G, N, Fn, Fe, dtype, n_nodes, nn_bytes, groups = _check_inputs(what, nodes, edges, n_nodes, groups, False)
    H = (N if max_n_nodes is None else int(max_n_nodes)) + 1
    if not 1 <= H <= L.ANALYZE_MAX_HIST + 1:
        raise ValueError(f"{what}: max_n_nodes must be in [0, {L.ANALYZE_MAX_HIST}]")
    if len(groups) == 3:
        if use_imp_H is None and use_chirality is None:
            use_imp_H, use_chirality = True, False
        elif use_imp_H is None:
            use_imp_H = not use_chirality
        elif use_chirality is None:
            use_chirality = not use_imp_H
        if bool(use_imp_H) == bool(use_chirality):
            raise ValueError(f"{what}: three groups hold exactly one of implicit H and chirality")
    else:
        use_imp_H = use_chirality = len(groups) == 4
    dev = nodes.device
    termination, term_dtype = _check_termination(what, termination, G, dev)
    nb = H + Fn + L.ANALYZE_EDGE_BINS + Fe
    out = torch.zeros(nb + 3, dtype=torch.float32, device=dev)
    if G > 0:
        totals = torch.zeros(nb + 2, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            L.check(L.load().gi_mol_properties(
                G, N, Fn, Fe, nodes.data_ptr(), edges.data_ptr(), dtype,
                None if n_nodes is None else n_nodes.data_ptr(), nn_bytes,
                None if termination is None else termination.data_ptr(), term_dtype, H - 1, totals.data_ptr(),
                out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "gi_mol_properties")
    col = out[H:H + Fn]
    off = np.cumsum([0] + groups).tolist()
    seg = [col[off[k]:off[k + 1]] for k in range(len(groups))]
    third = seg[2] if len(groups) >= 3 else None
    props = {
        "n_nodes_hist": out[:H],
        "avg_n_nodes": out[nb],
        "atom_type_hist": seg[0],
        "formal_charge_hist": seg[1],
        "n_edges_hist": out[H + Fn:H + Fn + L.ANALYZE_EDGE_BINS],
        "avg_n_edges": out[nb + 1],
        "edge_feature_hist": out[H + Fn + L.ANALYZE_EDGE_BINS:nb],
        "numh_hist": third if use_imp_H else [0] * int(n_imp_H),
        "chirality_hist": seg[-1] if use_chirality else [0] * int(n_chirality),
    }
    if termination is not None:
        props["fraction_properly_terminated"] = out[nb + 2]
    if epoch_key is not None:
        props = {(epoch_key, k): v for k, v in props.items()}
    return props


class DecodedMolecules(_ResultBuffer):
    """What ``decode`` wrote, on the device: ``atoms`` [G, N, S] int8, ``bonds`` [G, max_bonds, 3] int16, ``n_bonds``
    [G] int32 and ``status`` [G] int32; ``host()`` -> numpy ``(atoms, bonds, n_bonds, status)``."""

    def __init__(self, buf: torch.Tensor, G: int, N: int, S: int, max_bonds: int):
        super().__init__(buf, G, N, S, max_bonds)
        self.N, self.S, self.max_bonds = N, S, max_bonds

    @staticmethod
    @functools.lru_cache(maxsize=64)
    def layout(G: int, N: int, S: int, max_bonds: int) -> dict:
        return _pack(("status", "int32", (G,)), ("n_bonds", "int32", (G,)), ("bonds", "int16", (G, max_bonds, 3)),
                     ("atoms", "int8", (G, N, S)))

    @staticmethod
    def _host_result(a):
        return a["atoms"], a["bonds"], a["n_bonds"], a["status"]

    def molecule(self, i: int):
        """-> ``(atoms [n, S], bonds [min(n_bonds, max_bonds), 3], status)`` of graph ``i`` on the host, ``n`` being
        the rows that are not -1 throughout (``n_nodes`` unless a row below it is empty, status bit 1)."""
        atoms, bonds, n_bonds, status = self.host()
        a = atoms[i]
        live = np.flatnonzero((a >= 0).any(axis=1))
        n = int(live[-1]) + 1 if live.size else 0
        return a[:n], bonds[i, :min(int(n_bonds[i]), self.max_bonds)], int(status[i])


def decode(nodes: torch.Tensor, edges: torch.Tensor, n_nodes: torch.Tensor, groups: Sequence[int], *,
           max_bonds: Optional[int] = None, strict: bool = False) -> DecodedMolecules:
    """What ``graph_to_graph`` (GraphGenerator.py:659-804) reads out of the tensors, for all G graphs in one launch;
    inputs as ``molecular_properties`` (``n_nodes`` required).

    ``atoms`` [G, N, len(groups)] int8: for a node below ``n_nodes`` the index INSIDE each segment of that segment's
    set entry — for a well-formed row what ``_features_to_atom`` derives from ``nonzero_idc[0]``, ``[1]``, ``[2]``,
    ``[-1]`` minus the segment offsets (a segment with several set entries gives the first, one without gives -1) —
    and -1 for the other nodes.  ``bonds`` [G, max_bonds, 3] int16 (``max_bonds`` defaults to 2 N, padded with -1)
    and ``n_bonds`` [G]: the triples (i, j, bond type), i < j, of the non-zero entries of the whole N x N x Fe
    tensor in the order of ``torch.nonzero(edge_features * edge_mask)``.  ``status`` [G] int32, bits ``lib.MOL_*``:
    1 a node row below ``n_nodes`` is not one-hot per segment, 2 a bond touches a node >= ``n_nodes`` (the reference
    raises ``KeyError``), 4 more than ``max_bonds`` bonds (the first ``max_bonds`` are kept, ``n_bonds`` is the true
    count), 8 an entry is neither 0 nor 1, 16 a pair carries several bond types (all are emitted).

    Nothing is read back: ``.host()`` of the returned object does that with one copy and one synchronisation.
    ``strict=True`` does so at once and raises ``ValueError`` naming the first graph whose status is non-zero; the
    default only returns the status, because the generation loop's dummy graph 0 is legitimately malformed."""
    what = "decode"
    G, N, Fn, Fe, dtype, n_nodes, nn_bytes, groups = _check_inputs(what, nodes, edges, n_nodes, groups, True)
    if max(groups) > 127:
        raise ValueError(f"{what}: a segment of more than 127 entries does not fit the int8 atom records")
    mb = 2 * N if max_bonds is None else int(max_bonds)
    if not 1 <= mb <= 1 << 20:
        raise ValueError(f"{what}: max_bonds must be in [1, 2**20]")
    S = len(groups)
    dev = nodes.device
    res = DecodedMolecules.empty(dev, G, N, S, mb)
    if G > 0:
        seg, out = (C.c_int * S)(*groups), res._ptrs()
        with torch.cuda.device(dev):
            L.check(L.load().gi_mol_decode(
                G, N, Fn, Fe, nodes.data_ptr(), edges.data_ptr(), dtype, n_nodes.data_ptr(), nn_bytes, S, seg, mb,
                out["atoms"], out["bonds"], out["n_bonds"], out["status"],
                torch.cuda.current_stream(dev).cuda_stream), "gi_mol_decode")
    if strict:
        status = res.host()[3]
        bad = np.flatnonzero(status)
        if bad.size:
            g = int(bad[0])
            raise ValueError(f"decode: graph {g} (of {bad.size} with a non-zero status) has status {int(status[g])}: "
                             f"{describe_status(int(status[g]))}")
    return res


def records(decoded, atom_types: Sequence, formal_charge: Sequence, imp_H: Optional[Sequence] = None,
            chirality: Optional[Sequence] = None, int_to_bondtype=None) -> Iterator[tuple]:
    """Pure Python: per molecule ``(atoms, bonds)`` in the order ``_graph_to_mol`` (GraphGenerator.py:732-788) calls
    ``AddAtom`` and ``AddBond``.  ``atoms`` is a list of ``(symbol, formal_charge, total_num_h, cip_code)``, the
    arguments of ``Chem.Atom``, ``SetFormalCharge``, ``SetUnsignedProp("_TotalNumHs", .)`` and
    ``SetProp("_CIPCode", .)`` (``None`` where ``imp_H`` / ``chirality`` is not given, i.e. the reference makes no
    such call); ``bonds`` a list of ``(i, j, bond)`` with ``bond = int_to_bondtype[type]`` (the bare type index when
    no table is given).  ``decoded``: ``decode``'s result, or the ``(atoms, bonds, n_bonds, status)`` arrays of its
    ``.host()``.  The tables are the constants' ``atom_types``, ``formal_charge``, ``imp_H``, ``chirality`` and
    ``int_to_bondtype``; the optional ones must be given exactly for the segments that ``groups`` held.  An index of
    ``None`` instead of the pair is yielded for a graph with status bit 1 or 2: the reference's ``_graph_to_mol``
    misreads such a graph or raises on it (``IndexError``, which ``graph_to_graph`` turns into ``mol = None``, or
    ``KeyError``).  The generation loop's dummy graph 0 is such a graph."""
    atoms, bonds, n_bonds, status = decoded.host() if hasattr(decoded, "host") else decoded
    tables = [atom_types, formal_charge] + [t for t in (imp_H, chirality) if t is not None]
    if atoms.shape[2] != len(tables):
        raise ValueError(f"records: {atoms.shape[2]} segments were decoded but {len(tables)} tables are given")
    h_col = 2 if imp_H is not None else None
    c_col = len(tables) - 1 if chirality is not None else None
    for g in range(atoms.shape[0]):
        if int(status[g]) & (L.MOL_ONEHOT | L.MOL_BOND_PAST_N):
            yield None
            continue
        mol_atoms = []
        for row in atoms[g].tolist():
            if row[0] < 0:
                break                                   # past n_nodes
            mol_atoms.append((atom_types[row[0]], formal_charge[row[1]],
                              None if h_col is None else imp_H[row[h_col]],
                              None if c_col is None else chirality[row[c_col]]))
        kept = min(int(n_bonds[g]), bonds.shape[1])
        mol_bonds = [(i, j, t if int_to_bondtype is None else int_to_bondtype[t]) for i, j, t in bonds[g, :kept].tolist()]
        yield mol_atoms, mol_bonds


# ---- molecule identity -------------------------------------------------------------------------------------------
#: status bits of ``canonical`` beyond ``STATUS_MESSAGES``' MOL_BOND_PAST_N and MOL_VALUE
CANON_STATUS_MESSAGES = {
    L.MOL_BOND_PAST_N: STATUS_MESSAGES[L.MOL_BOND_PAST_N],
    L.MOL_VALUE: STATUS_MESSAGES[L.MOL_VALUE],
    L.MOL_ASYMMETRIC: "edges[i, j, t] is set and edges[j, i, t] is not",
    L.MOL_NODE_PAST_N: "a node row >= n_nodes has a set entry, or n_nodes is outside [0, N]",
}


class CanonicalMolecules(_ResultBuffer):
    """What ``canonical`` wrote, on the device: ``order`` / ``rank`` [G, N] int32, ``key`` [G, 2] int64 (the two
    64-bit words of the key, as torch has no uint64 arithmetic; ``host()`` gives uint64), ``status`` [G] int32;
    ``host()`` -> numpy ``(order, rank, key, status)``.  And, if asked for, ``nodes`` [G, N, Fn] / ``edges``
    [G, N, N, Fe] int8, the canonical molecules (``None`` otherwise; not part of ``host()``)."""

    _HOST_DTYPE = {"key": "uint64"}

    def __init__(self, buf: torch.Tensor, G: int, N: int, nodes=None, edges=None):
        super().__init__(buf, G, N)
        self.N, self.nodes, self.edges = N, nodes, edges

    @staticmethod
    @functools.lru_cache(maxsize=64)
    def layout(G: int, N: int) -> dict:
        return _pack(("key", "int64", (G, 2)), ("order", "int32", (G, N)), ("rank", "int32", (G, N)),
                     ("status", "int32", (G,)))

    @staticmethod
    def _host_result(a):
        return a["order"], a["rank"], a["key"], a["status"]


def canonical(nodes: torch.Tensor, edges: torch.Tensor, n_nodes: Optional[torch.Tensor] = None, *,
              want_molecules: bool = False) -> CanonicalMolecules:
    """A canonical node order, the canonical form and a 128-bit key of every molecule, in one launch
    (``gi_mol_canon``); inputs as ``molecular_properties`` (no ``groups``; ``n_nodes = None`` takes the number of
    LEADING node rows with a set entry, the convention of ``routes.check``).  The nodes may be in any order.

    WHAT IDENTITY MEANS: two molecules are equal iff their labelled graphs are isomorphic — node feature rows and bond
    types, nothing else.  The reference compares canonical SMILES after RDKit's sanitisation, so a Kekule and an
    aromatic encoding of one compound are equal there and DIFFERENT here; two tensors that differ only in the order of
    the nodes are equal in both.

    ``order[g, a]`` is the input index of canonical position ``a`` (-1 past n), ``rank`` its inverse; the canonical
    molecule is ``nodes[order]``, ``edges[order][:, order]``, zero padded (``want_molecules=True`` returns it as int8
    ``.nodes`` / ``.edges``); ``key`` is a hash of it (include/graphinvent_amd.h has the algorithm, tests/canon_model.py
    a numpy version).  ``status``: 0, or ``lib.MOL_VALUE | MOL_BOND_PAST_N | MOL_ASYMMETRIC | MOL_NODE_PAST_N``
    (``CANON_STATUS_MESSAGES``); such a molecule keeps the identity order, gets a zero form and a key of its own.

    COMPLETENESS: the order comes from colour refinement with individualisation and NO backtracking.  Equal forms
    always mean isomorphic graphs.  The converse holds when every refinement cell is an orbit of the automorphism
    group (every molecule of the fixtures; rings, cages such as cubane, adamantane or dodecahedrane); a graph with a
    cell that is not an orbit (the Frucht graph, the Shrikhande graph, a disconnected C6 + 2 C3) can come out in
    several forms, so two copies of it in different node orders may count as distinct.  The error is always towards
    "unique".  Nothing is read back: ``.host()`` does that with one copy and one synchronisation."""
    what = "canonical"
    G, N, Fn, Fe, dtype, n_nodes, nn_bytes, _ = _check_inputs(what, nodes, edges, n_nodes, None, False)
    dev = nodes.device
    cn = ce = None
    if want_molecules:
        cn = torch.empty((G, N, Fn), dtype=torch.int8, device=dev)
        ce = torch.empty((G, N, N, Fe), dtype=torch.int8, device=dev)
    res = CanonicalMolecules.empty(dev, G, N, nodes=cn, edges=ce)
    if G > 0:
        out = res._ptrs()
        with torch.cuda.device(dev):
            L.check(L.load().gi_mol_canon(
                G, N, Fn, Fe, nodes.data_ptr(), edges.data_ptr(), dtype,
                None if n_nodes is None else n_nodes.data_ptr(), nn_bytes, out["order"], out["rank"], out["key"],
                out["status"], None if cn is None else cn.data_ptr(),
                None if ce is None else ce.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "gi_mol_canon")
    return res


def _check_mask(what: str, mask, G: int, dev):
    if mask is None:
        return None
    if not isinstance(mask, torch.Tensor) or not mask.is_cuda or mask.device != dev:
        raise RuntimeError(f"{what}: mask must be a CUDA tensor on {dev} (no CPU fallback)")
    if tuple(mask.shape) != (G,):
        raise ValueError(f"{what}: mask has shape {tuple(mask.shape)}, expected ({G},)")
    return (mask != 0).to(torch.int8)


def _unique(what: str, nodes, edges, n_nodes, mask):
    """-> (canonical molecules, uniqueness, rep, counts) on the device."""
    G, N = _check_inputs(what, nodes, edges, n_nodes, None, False)[:2]      # everything is checked before a launch
    dev = nodes.device
    mask = _check_mask(what, mask, G, dev)
    can = canonical(nodes, edges, n_nodes, want_molecules=True)
    lib = L.load()
    uniq = torch.empty(G, dtype=torch.float32, device=dev)
    rep = torch.empty(G, dtype=torch.int32, device=dev)
    counts = torch.empty(L.MOL_COUNTS, dtype=torch.int32, device=dev)
    ws = torch.empty(max(int(lib.gi_mol_unique_ws_bytes(G)), 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.gi_mol_unique(
            G, N, nodes.shape[2], edges.shape[3], can.key.data_ptr(), can.nodes.data_ptr(), can.edges.data_ptr(),
            can.status.data_ptr(), None if mask is None else mask.data_ptr(), ws.data_ptr(), rep.data_ptr(),
            uniq.data_ptr(), counts.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "gi_mol_unique")
    return can, uniq, rep, counts


def unique(nodes: torch.Tensor, edges: torch.Tensor, n_nodes: Optional[torch.Tensor] = None, *,
           mask: Optional[torch.Tensor] = None):
    """The reference's ``uniqueness_tensor`` (util.py:549-585) for a batch of generated graphs, without a SMILES
    string and without a read-back: ``(uniqueness, rep, n_classes)``.

    ``uniqueness`` [G] fp32 is 0 exactly where ``mask[i]`` is set and an earlier masked-in molecule ``j < i`` is the
    same molecule (``canonical``'s identity, decided by comparing the canonical bytes), 1 elsewhere: it drops into
    ``Workflow.compute_loss_component`` / ``ScoringFunction.compute_score`` in place of the reference's tensor.
    ``mask`` [G] (any dtype, non-zero = in; default all) plays the part of the reference's validity: a masked-out
    molecule keeps 1 and is not remembered.  ``rep`` [G] int32: the lowest index of the molecule's class (-1 where
    masked out) — ``rep == arange(G)`` picks one representative per distinct graph.  ``n_classes``: a 0-d int32 device
    tensor, the number of classes among the masked-in molecules.  A malformed molecule (``canonical``'s status) is a
    class of its own."""
    _, uniq, rep, counts = _unique("unique", nodes, edges, n_nodes, mask)
    return uniq, rep, counts[2]


def fraction_unique(nodes: torch.Tensor, edges: torch.Tensor, n_nodes: Optional[torch.Tensor] = None, *,
                    mask: Optional[torch.Tensor] = None) -> float:
    """``Analyzer._get_fraction_unique``'s quotient (Analyzer.py:494-496): distinct molecules among the masked-in
    (valid) ones divided by ALL G, under ``canonical``'s identity.  One read-back; G = 0 gives 0."""
    can, _, _, counts = _unique("fraction_unique", nodes, edges, n_nodes, mask)
    G = can.G
    if G == 0:
        return 0.0
    with _host_sync_allowed():
        return int(counts[2].item()) / G


class SeenSet:
    """Molecules seen so far, across calls: "unique over a whole generation epoch", or "novel against the training
    set" (add the training molecules first).  A device table of ``capacity`` (a power of two) 128-bit keys of
    ``canonical``; the molecules themselves are not kept, so ACROSS CALLS EQUALITY IS BY KEY, not by bytes (inside one
    call it is by bytes, as in ``unique``): two different molecules with one key, a 2**-128 accident per pair, would
    count as one.  Keep the table at most half full: a probe is linear."""

    def __init__(self, capacity: int, device="cuda"):
        capacity = int(capacity)
        if capacity < 1 or capacity & (capacity - 1):
            raise ValueError(f"SeenSet: capacity must be a power of two, got {capacity}")
        self.capacity, self.device = capacity, torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"SeenSet needs a CUDA (ROCm) device, got {self.device}: the MI355X HIP path has no CPU "
                               "fallback")
        self._table = torch.zeros((capacity, 2), dtype=torch.int64, device=self.device)
        self._info = torch.zeros(2, dtype=torch.int32, device=self.device)
        self._dims = None

    def add(self, nodes: torch.Tensor, edges: torch.Tensor, n_nodes: Optional[torch.Tensor] = None,
            mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """-> ``new`` [G] int32, no read-back: 1 for the first masked-in occurrence (inside this call) of a molecule
        whose key was not in the table, which now holds it; 0 for later copies, masked-out molecules and molecules
        seen in an earlier call.  A malformed masked-in molecule gets 1 and is not stored.  When the table is full,
        ``overflowed()`` turns true, nothing more is stored and unseen molecules keep reporting 1."""
        what = "SeenSet.add"
        dims = _check_inputs(what, nodes, edges, n_nodes, None, False)[1:4]
        if nodes.device != self._table.device:
            raise ValueError(f"{what}: the molecules are on {nodes.device}, the table on {self._table.device}")
        if self._dims not in (None, dims):
            raise ValueError(f"{what}: (N, Fn, Fe) = {dims}, the table holds keys of {self._dims}")
        can, _, rep, _ = _unique(what, nodes, edges, n_nodes, mask)
        self._dims = dims
        new = torch.empty(can.G, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            L.check(L.load().gi_mol_seen_add(
                can.G, can.key.data_ptr(), can.status.data_ptr(), rep.data_ptr(), self._table.data_ptr(),
                self.capacity, self._info.data_ptr(), new.data_ptr(),
                torch.cuda.current_stream(self.device).cuda_stream), "gi_mol_seen_add")
        return new

    def _read(self):
        with _host_sync_allowed():
            return self._info.tolist()

    def count(self) -> int:
        """Keys in the table (one read-back)."""
        return int(self._read()[0])

    def overflowed(self) -> bool:
        """Whether a key ever found the table full (sticky; one read-back)."""
        return bool(self._read()[1] & L.SEEN_FULL)


# ---- molecule validity -------------------------------------------------------------------------------------------
#: (period, group) of the elements the default table knows; hydrogen is handled apart
_ELEMENTS = {"B": (2, 13), "C": (2, 14), "N": (2, 15), "O": (2, 16), "F": (2, 17), "Si": (3, 14), "P": (3, 15),
             "S": (3, 16), "Cl": (3, 17), "Se": (4, 16), "Br": (4, 17), "I": (5, 17)}
#: allowed total valences of a NEUTRAL atom by group: the first row (period 2), and the rows below it
_GROUP_VALENCES = {2: {13: (3,), 14: (4,), 15: (3,), 16: (2,), 17: (1,), 18: (0,)},
                   3: {13: (3,), 14: (4,), 15: (3, 5), 16: (2, 4, 6), 17: (1,), 18: (0,)}}
#: standard atomic weights in millidalton
DEFAULT_MASSES = {"H": 1008, "B": 10810, "C": 12011, "N": 14007, "O": 15999, "F": 18998, "Si": 28085, "P": 30974,
                  "S": 32060, "Cl": 35450, "Se": 78971, "Br": 79904, "I": 126904}
_BOND_ORDER2 = {1: 2, 1.5: 3, 2: 4, 3: 6}

#: status bits of ``validity`` that make a molecule invalid, and the informational ones
VALIDITY_STATUS_MESSAGES = {
    L.MOL_ONEHOT: "a node row below n_nodes does not have exactly one set entry in the atom type, formal charge or "
                  "implicit-H segment",
    L.MOL_BOND_PAST_N: STATUS_MESSAGES[L.MOL_BOND_PAST_N],
    L.MOL_VALUE: STATUS_MESSAGES[L.MOL_VALUE],
    L.MOL_MULTI_BOND: STATUS_MESSAGES[L.MOL_MULTI_BOND],
    L.MOL_ASYMMETRIC: CANON_STATUS_MESSAGES[L.MOL_ASYMMETRIC],
    L.MOL_NODE_PAST_N: CANON_STATUS_MESSAGES[L.MOL_NODE_PAST_N],
    L.VAL_EMPTY: "the molecule has no atoms (the reference's mol = None)",
    L.VAL_SELF_LOOP: "an atom is bonded to itself (RDKit's AddBond refuses it)",
    L.VAL_OVER: "an atom has more bonds than any allowed valence of its element and charge",
    L.VAL_FRAGMENTS: "more than one connected component (invalid only with require_connected)",
    L.VAL_AROMATIC: "a bond of order 1.5 is present: counted 3 per 2, NOT kekulised (informational)",
    L.VAL_H_MISMATCH: "a stored implicit-H count differs from the hydrogen fill (informational)",
}
MALFORMED_BITS = (L.MOL_ONEHOT | L.MOL_BOND_PAST_N | L.MOL_VALUE | L.MOL_MULTI_BOND | L.MOL_ASYMMETRIC |
                  L.MOL_NODE_PAST_N)
INVALID_BITS = MALFORMED_BITS | L.VAL_EMPTY | L.VAL_SELF_LOOP | L.VAL_OVER


def default_valences(symbol: str, charge: int):
    """The default table's allowed total valences of ``symbol`` with formal charge ``charge``, or ``None`` where the
    table has no entry.  OURS, NOT CHECKED AGAINST RDKit.  Neutral atoms: H 1; B 3; C, Si 4; N 3; P 3, 5; O 2; S, Se
    2, 4, 6; F, Cl, Br, I 1; a noble gas 0.  An atom of group g with charge c in {-1, 0, +1} takes the list of group
    g - c of its own period (period 2 the first-row lists, lower periods those of P / S): N+ 4, O+ 3, N- 2, O- 1,
    C- 3, C+ 3, B- 4, S+ 3 / 5, Cl- 0, Cl+ 2 / 4 / 6.  H+ and H- are 0."""
    if charge not in (-1, 0, 1):
        return None
    if symbol == "H":
        return (1,) if charge == 0 else (0,)
    if symbol not in _ELEMENTS:
        return None
    period, group = _ELEMENTS[symbol]
    return _GROUP_VALENCES[2 if period == 2 else 3].get(group - charge)


class ValenceRules:
    """The tables ``validity`` judges by, built once and kept on the device.

    ``atom_types`` (symbols), ``formal_charge`` (integers) and ``imp_H`` (hydrogen counts; ``None``: no implicit-H
    segment) are the constants' lists in the node row's segment order; whatever follows them in a node row (a
    chirality segment) is ignored.  ``bond_orders``: the order of every bond type, from {1, 1.5, 2, 3}; without it
    edges of three bond types are read as ``(1, 2, 3)`` and of four as ``(1, 2, 3, 1.5)`` (the reference's
    ``bondtype_to_int`` order), and any other number of bond types raises ``ValueError`` in ``validity``.  ``allowed``
    ``{(symbol, charge): (valences, ...)}`` overrides or extends the default table (``default_valences``, which is
    ours and NOT CHECKED AGAINST RDKit) per entry; a combination of ``atom_types`` x ``formal_charge`` that neither
    has raises ``ValueError``.  ``masses`` ``{symbol: millidalton}`` overrides ``DEFAULT_MASSES``.

    Device tables: ``allowed_mask`` [A * C] int16 (bit v = total valence v allowed, 0..15), ``mass`` [A] int32
    (millidalton), ``order2(Fe)`` [Fe] int8 (twice the bond order), ``h_values`` [H] int8; their host copies are
    ``mask_table`` [A, C] uint16, ``mass_table`` and ``order2_tables``, and ``valences`` maps (symbol, charge) to the
    tuple.  ``device=None`` builds the host copies only (for inspection; ``validity`` refuses such rules)."""

    def __init__(self, atom_types: Sequence[str], formal_charge: Sequence[int], *, imp_H: Optional[Sequence[int]] = None,
                 bond_orders: Optional[Sequence[float]] = None, allowed: Optional[dict] = None,
                 masses: Optional[dict] = None, device="cuda"):
        self.atom_types, self.formal_charge = [str(a) for a in atom_types], [int(c) for c in formal_charge]
        self.imp_H = None if imp_H is None else [int(h) for h in imp_H]
        if not self.atom_types or not self.formal_charge or (self.imp_H is not None and not self.imp_H):
            raise ValueError("ValenceRules: atom_types, formal_charge and (if given) imp_H must not be empty")
        if self.imp_H is not None and not all(0 <= h <= 127 for h in self.imp_H):
            raise ValueError(f"ValenceRules: imp_H {self.imp_H} must hold hydrogen counts in [0, 127]")
        if bond_orders is not None:
            if not 1 <= len(bond_orders) <= L.GI_MAX_GROUPS:
                raise ValueError(f"ValenceRules: 1 to {L.GI_MAX_GROUPS} bond types, got {len(bond_orders)}")
            for b in bond_orders:
                if b not in _BOND_ORDER2:
                    raise ValueError(f"ValenceRules: bond order {b!r} is not one of 1, 1.5, 2, 3")
        self.bond_orders = None if bond_orders is None else tuple(bond_orders)
        allowed = dict(allowed or {})
        for key, vals in allowed.items():
            if (not isinstance(key, tuple) or len(key) != 2 or not all(isinstance(v, (int, np.integer)) and 0 <= v <= 15
                                                                       for v in vals)):
                raise ValueError(f"ValenceRules: allowed[{key!r}] = {vals!r} must map (symbol, charge) to valences in "
                                 "[0, 15]")
        mass_of = dict(DEFAULT_MASSES)
        mass_of.update({str(k): int(v) for k, v in (masses or {}).items()})
        self.valences = {}
        masks = []
        for a in self.atom_types:
            if a not in mass_of:
                raise ValueError(f"ValenceRules: no mass for element {a!r}; give masses={{{a!r}: millidalton}}")
            for c in self.formal_charge:
                vals = allowed[(a, c)] if (a, c) in allowed else default_valences(a, c)
                if vals is None:
                    raise ValueError(f"ValenceRules: no allowed valences for element {a!r} with formal charge {c:+d}; "
                                     f"give allowed={{({a!r}, {c}): (valences, ...)}}")
                self.valences[(a, c)] = tuple(sorted(int(v) for v in vals))
                masks.append(sum(1 << v for v in set(self.valences[(a, c)])))
        if "H" not in mass_of:
            raise ValueError("ValenceRules: masses must keep an entry for 'H'")
        self.masses = {a: mass_of[a] for a in self.atom_types}
        self.mass_h = mass_of["H"]
        self.h_type = self.atom_types.index("H") if "H" in self.atom_types else -1
        self.groups = (len(self.atom_types), len(self.formal_charge), len(self.imp_H or ()))
        self.mask_table = np.array(masks, np.uint16).reshape(self.groups[0], self.groups[1])
        self.mass_table = np.array([self.masses[a] for a in self.atom_types], np.int32)
        sets = [(1, 2, 3), (1, 2, 3, 1.5)] if self.bond_orders is None else [self.bond_orders]
        self.order2_tables = {len(bo): np.array([_BOND_ORDER2[b] for b in bo], np.int8) for bo in sets}
        self.device = None if device is None else torch.device(device)
        self.allowed_mask = self.mass = self.h_values = None
        self._order2, self._scratch = {}, {}
        if self.device is None:
            return
        if self.device.type != "cuda":
            raise RuntimeError(f"ValenceRules needs a CUDA (ROCm) device, got {self.device}: the MI355X HIP path has no "
                               "CPU fallback (device=None keeps the tables on the host, for inspection only)")
        self.allowed_mask = torch.from_numpy(self.mask_table.view(np.int16).reshape(-1)).to(self.device)
        self.mass = torch.from_numpy(self.mass_table).to(self.device)
        self._order2 = {k: torch.from_numpy(v).to(self.device) for k, v in self.order2_tables.items()}
        if self.imp_H is not None:
            self.h_values = torch.tensor(self.imp_H, dtype=torch.int8, device=self.device)

    def scratch(self, stream: int) -> torch.Tensor:
        """The counters' scratch words of ``gi_mol_valence`` for calls issued on ``stream`` (zero between calls)."""
        if stream not in self._scratch:
            self._scratch[stream] = torch.zeros(L.VAL_SCRATCH, dtype=torch.int32, device=self.device)
        return self._scratch[stream]

    def order2(self, Fe: int) -> torch.Tensor:
        """Twice the bond order of each of ``Fe`` bond types, int8, on the device."""
        if Fe not in self.order2_tables:
            if self.bond_orders is None:
                raise ValueError(f"ValenceRules: bond_orders is required for {Fe} bond types (the defaults cover three: "
                                 "1, 2, 3 and four: 1, 2, 3, 1.5)")
            raise ValueError(f"ValenceRules: the rules hold {len(self.bond_orders)} bond orders, edges has Fe = {Fe}")
        return self._order2[Fe]


def _rules_groups(what: str, rules) -> tuple:
    """-> ``rules.groups``.  Every entry point asks this first, before it looks at a tensor: the ``TypeError`` wins."""
    if not isinstance(rules, ValenceRules):
        raise TypeError(f"{what}: rules must be a ValenceRules, got {type(rules).__name__}")
    return rules.groups


def _check_rules(what: str, rules, Fn: int, Fe: int, dev):
    """``rules`` (which ``_rules_groups`` has seen) against inputs of ``Fn`` node entries and ``Fe`` bond types on
    ``dev`` -> (A, C, H, order2 on the device).  ``dev = None``: the caller does not know the inputs' device yet and
    compares it itself."""
    A, Cn, H = rules.groups
    if A + Cn + H > Fn:
        raise ValueError(f"{what}: the rules' segments {rules.groups} do not fit node rows of Fn = {Fn}")
    if rules.device is None:
        raise RuntimeError(f"{what}: the rules were built with device=None and hold no device tables (no CPU fallback)")
    order2 = rules.order2(Fe)
    if dev is not None and order2.device != dev:
        raise ValueError(f"{what}: the molecules are on {dev}, the rules' tables on {order2.device}")
    return A, Cn, H, order2


class MoleculeValidity(_ResultBuffer):
    """What ``validity`` wrote, on the device: ``valid`` [G] fp32, ``status`` / ``first_bad`` [G] int32,
    ``atom_valence`` / ``atom_h`` [G, N] int8, ``desc`` [G, 6] int32 (``DESC_NAMES``) and ``counts`` [4] int32 (valid,
    terminated, valid and terminated, G); ``host()`` -> ``{name: numpy array}`` of all seven."""

    DESC_NAMES = ("n_atoms", "n_h", "mass_mda", "n_bonds", "n_components", "n_rings")

    def __init__(self, buf: torch.Tensor, G: int, N: int):
        super().__init__(buf, G, N)
        self.N = N

    @staticmethod
    @functools.lru_cache(maxsize=64)
    def layout(G: int, N: int) -> dict:
        """name -> (byte offset, bytes, dtype name, shape) inside the buffer; every array is aligned to itself."""
        return _pack(("counts", "int32", (L.VAL_COUNTS,)), ("status", "int32", (G,)), ("first_bad", "int32", (G,)),
                     ("valid", "float32", (G,)), ("desc", "int32", (G, L.VAL_DESC)), ("atom_valence", "int8", (G, N)),
                     ("atom_h", "int8", (G, N)))

    @staticmethod
    def _host_result(a):
        return a


def validity(nodes: torch.Tensor, edges: torch.Tensor, n_nodes: Optional[torch.Tensor], rules: ValenceRules, *,
             termination: Optional[torch.Tensor] = None, require_connected: bool = False) -> MoleculeValidity:
    """The reference's ``validity_tensor`` (util.py:549-585; ``fraction_valid``, Analyzer.py:501-544) for all G
    molecules in one launch (``gi_mol_valence``), with no RDKit and no read-back; inputs as ``canonical``
    (``n_nodes = None``: the leading node rows with a set entry), the node row's segments from ``rules``.

    **THIS IS A VALENCE TEST OF THE LABELLED GRAPH, NOT RDKit's SANITISATION.**  What ``SanitizeMol`` can reject for
    the default bond set (single / double / triple) is an atom with more bonds than its element and charge allow;
    that, a table look-up per atom, is what is judged here, by ``rules``' table, which is ours.  **No kekulisation or
    aromaticity perception is done**: a bond of order 1.5 counts 3 per 2 and raises ``VAL_AROMATIC``, so that the
    caller can route such molecules to RDKit.

    Per atom i < n, in integers: ``o2 = sum_t order2[t] * #{j : edges[i, j, t]}``, ``x = ceil(o2 / 2)``, ``v*`` the
    smallest allowed valence >= x; without one the atom is over its valence, otherwise its hydrogen fill is
    ``h = v* - x``.  An implicit-H segment does not enter the verdict (the reference stores it only as the
    ``_TotalNumHs`` property, which sanitisation does not read); it is compared with the fill (``VAL_H_MISMATCH``).

    Result (``MoleculeValidity``, views of one device buffer; ``.host()`` is one copy and one synchronisation):
    ``valid`` [G] fp32, 1 / 0, drops into ``ScoringFunction.compute_score`` and ``unique(..., mask=valid)``;
    ``status`` [G] int32 (``VALIDITY_STATUS_MESSAGES``: the ``lib.MOL_*`` bits of a malformed molecule, ``VAL_EMPTY``,
    ``VAL_SELF_LOOP``, ``VAL_OVER`` — all invalidating — and ``VAL_FRAGMENTS`` (invalidating only with
    ``require_connected``: sanitisation accepts fragments), ``VAL_AROMATIC``, ``VAL_H_MISMATCH``); ``first_bad`` [G]
    the lowest atom over its valence (-1: none); ``atom_valence`` [G, N] int8 = min(x, 127) and ``atom_h`` [G, N] int8
    = the fill (0 for an atom over its valence), both -1 past n and throughout a malformed molecule, for which nothing
    beyond the malformed bits, ``VAL_EMPTY`` and ``VAL_SELF_LOOP`` is evaluated and ``desc`` is zero; ``desc`` [G, 6]
    int32 = n_atoms, n_h (fills + atoms of type "H"), mass_mda (``sum mass[type] + fills * mass_H``), n_bonds (pairs
    i < j with a bond), n_components, n_rings (= n_bonds - n_atoms + n_components); ``counts`` [4] int32 = valid,
    terminated (``termination`` [G] non-zero; none given: 0), valid and terminated, G."""
    what = "validity"
    _rules_groups(what, rules)
    G, N, Fn, Fe, dtype, n_nodes, nn_bytes, _ = _check_inputs(what, nodes, edges, n_nodes, None, False)
    dev = nodes.device
    A, Cn, H, order2 = _check_rules(what, rules, Fn, Fe, dev)
    termination, term_dtype = _check_termination(what, termination, G, dev)
    if G == 0:                                               # no launch: the counts are zero
        return MoleculeValidity(torch.zeros(MoleculeValidity.nbytes(0, N), dtype=torch.uint8, device=dev), 0, N)
    res = MoleculeValidity.empty(dev, G, N)
    out = res._ptrs()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        L.check(L.load().gi_mol_valence(
            G, N, Fn, Fe, nodes.data_ptr(), edges.data_ptr(), dtype,
            None if n_nodes is None else n_nodes.data_ptr(), nn_bytes, A, Cn, H, rules.allowed_mask.data_ptr(),
            rules.mass.data_ptr(), order2.data_ptr(), None if rules.h_values is None else rules.h_values.data_ptr(),
            rules.h_type, rules.mass_h, None if termination is None else termination.data_ptr(), term_dtype,
            int(bool(require_connected)), out["valid"], out["status"], out["first_bad"], out["atom_valence"],
            out["atom_h"], out["desc"], out["counts"], rules.scratch(stream).data_ptr(), stream), "gi_mol_valence")
    return res


def fraction_valid(nodes, edges=None, n_nodes=None, rules=None, *, termination=None, require_connected=False):
    """``Analyzer._get_fraction_valid``'s three quotients (Analyzer.py:532-541) from ``validity``'s ``counts``:
    ``(fraction_valid, fraction_valid_properly_terminated, fraction_properly_terminated)`` as 0-d fp32 device tensors,
    with no read-back.  Takes ``validity``'s arguments, or its result as the only argument.  The reference's quirk is
    kept: ``fraction_valid_properly_terminated`` is 0.0 when nothing is terminated.  G = 0 gives zeros (the reference
    raises)."""
    res = nodes if isinstance(nodes, MoleculeValidity) else \
        validity(nodes, edges, n_nodes, rules, termination=termination, require_connected=require_connected)
    c = res.counts.to(torch.float32)
    zero = torch.zeros((), dtype=torch.float32, device=c.device)
    some = c[3] > 0
    return (torch.where(some, c[0] / c[3], zero), torch.where(c[1] > 0, c[2] / c[1], zero),
            torch.where(some, c[1] / c[3], zero))


# ---- molecule scores: fingerprints, similarity, activity ----------------------------------------------------------
_FP_KINDS = {"tanimoto": L.FP_TANIMOTO, "rbf": L.FP_RBF, "linear": L.FP_LINEAR}


def _check_n_bits(what: str, n_bits) -> int:
    if (not isinstance(n_bits, (int, np.integer)) or isinstance(n_bits, bool)
            or not L.FP_MIN_BITS <= n_bits <= L.FP_MAX_BITS or n_bits & (n_bits - 1)):
        raise ValueError(f"{what}: n_bits must be a power of two in [{L.FP_MIN_BITS}, {L.FP_MAX_BITS}], got {n_bits!r}")
    return int(n_bits)


class Fingerprints(_ResultBuffer):
    """What ``fingerprint`` wrote, on the device: ``bits`` [G, n_bits / 32] int32 (bit b of a row is bit ``b & 31`` of
    word ``b >> 5``), ``popcount`` / ``status`` [G] int32 and, if asked for, ``atom_id`` [G, N, 2] int32 (the low and
    high halves of every atom's last identifier, -1 past n; ``None`` otherwise); ``host()`` -> ``{name: numpy array}``."""

    def __init__(self, buf: torch.Tensor, G: int, N: int, W: int, ids: bool):
        super().__init__(buf, G, N, W, ids)
        self.N, self.n_bits = N, 32 * W
        if not ids:
            self.atom_id = None

    @staticmethod
    @functools.lru_cache(maxsize=64)
    def layout(G: int, N: int, W: int, ids: bool) -> dict:
        return _pack(("bits", "int32", (G, W)), ("popcount", "int32", (G,)), ("status", "int32", (G,)),
                     *([("atom_id", "int32", (G, N, 2))] if ids else []))

    @staticmethod
    def _host_result(a):
        return a


def fingerprint(nodes: torch.Tensor, edges: torch.Tensor, n_nodes: Optional[torch.Tensor], rules: ValenceRules, *,
                radius: int = 2, n_bits: int = 2048, atom_ids: bool = False) -> Fingerprints:
    """A packed circular fingerprint of every molecule in one launch (``gi_mol_fingerprint``), with no RDKit and no
    read-back; inputs as ``validity`` (the node row's segments and the bond orders from ``rules``).

    **THIS IS A MORGAN-STYLE FINGERPRINT OF THE LABELLED GRAPH, NOT RDKit's ECFP BITS.**  The atom invariants differ (atom
    type, formal charge, number of bonded partners, twice the bond-order sum; **no ring membership, no isotope,
    hydrogens only through the bond-order sum**), the hash differs, **duplicate substructures are not removed and no
    aromaticity is perceived**.  A QSAR model must be trained on THESE fingerprints, which this function produces for any
    stored int8 molecules (``routes.molecules_from_rows``).  Guaranteed: two isomorphic labelled molecules get equal rows
    in any node order, and two atoms get equal identifiers after round r exactly when their radius-r labelled
    neighbourhoods are 1-WL-equivalent (up to 64-bit hash collisions).

    Per atom i < n, in 64-bit wrap-around integers (``tests/fingerprint_model.py`` is the numpy specification):
    ``id_0 = mix64(K0 + type + 256 charge + 2**16 degree + 2**24 o2)``, then for r = 1 .. ``radius`` (0 to 4)
    ``id_r[i] = mix64(mix64(id_{r-1}[i] + r) + sum over bonds (t, j) of mix64(id_{r-1}[j] ^ K1 order2[t]))``; bit
    ``id_r[i] & (n_bits - 1)`` of the row is set for every r and i.  ``n_bits``: a power of two in [64, 4096].

    ``status`` [G]: 0, or the malformed bits of ``validity`` (``MALFORMED_BITS``), ``VAL_EMPTY``, ``VAL_SELF_LOOP``; such
    a molecule gets an ALL-ZERO row (and scores 0 in ``activity``: the reference's ``except: pass``).  ``.host()`` is one
    copy and one synchronisation.  G = 0 is answered without a launch."""
    what = "fingerprint"
    _rules_groups(what, rules)
    n_bits = _check_n_bits(what, n_bits)
    if not isinstance(radius, (int, np.integer)) or isinstance(radius, bool) or not 0 <= radius <= L.FP_MAX_RADIUS:
        raise ValueError(f"{what}: radius must be an integer in [0, {L.FP_MAX_RADIUS}], got {radius!r}")
    G, N, Fn, Fe, dtype, n_nodes, nn_bytes, _ = _check_inputs(what, nodes, edges, n_nodes, None, False)
    dev = nodes.device
    A, Cn, H, order2 = _check_rules(what, rules, Fn, Fe, dev)
    W = n_bits // 32
    res = Fingerprints.empty(dev, G, N, W, bool(atom_ids))
    if G > 0:
        out = res._ptrs()
        with torch.cuda.device(dev):
            L.check(L.load().gi_mol_fingerprint(
                G, N, Fn, Fe, nodes.data_ptr(), edges.data_ptr(), dtype,
                None if n_nodes is None else n_nodes.data_ptr(), nn_bytes, A, Cn, H, order2.data_ptr(), int(radius),
                n_bits, out["bits"], out["popcount"], out["status"], out.get("atom_id"),
                torch.cuda.current_stream(dev).cuda_stream), "gi_mol_fingerprint")
    return res


def _pack_bits(what: str, bits) -> torch.Tensor:
    """Packed int32 [S, W] (kept) or a 0 / 1 array [S, n_bits] of any other dtype (packed here, on the host) ->
    a host int32 tensor [S, W]."""
    if isinstance(bits, torch.Tensor):
        if bits.dtype == torch.int32:
            arr = bits
        else:
            arr = bits.detach().cpu().numpy()
    else:
        arr = np.asarray(bits)
    if isinstance(arr, np.ndarray):
        if arr.dtype == np.int32:
            arr = torch.from_numpy(np.ascontiguousarray(arr))
        else:
            if arr.ndim != 2:
                raise ValueError(f"{what}: bits must be [S, n_bits] (0 / 1) or packed int32 [S, n_bits / 32]")
            _check_n_bits(what, arr.shape[1])
            if not np.isin(arr, (0, 1)).all():
                raise ValueError(f"{what}: an unpacked array must hold only 0 and 1")
            packed = np.packbits(arr != 0, axis=1, bitorder="little")
            arr = torch.from_numpy(np.ascontiguousarray(packed).view(np.int32))
    if arr.dim() != 2:
        raise ValueError(f"{what}: bits must be [S, n_bits] (0 / 1) or packed int32 [S, n_bits / 32]")
    _check_n_bits(what, 32 * arr.shape[1])
    return arr


class FingerprintSet:
    """A stored set of fingerprints on the device (actives, a training set, a model's support vectors): ``bits``
    [S, n_bits / 32] int32.  Built from packed int32 rows (a tensor or array of dtype int32, e.g. ``Fingerprints.bits``),
    or from a 0 / 1 array [S, n_bits] of ANY OTHER dtype, which is packed on the host once.  S >= 1."""

    def __init__(self, bits, device="cuda"):
        what = "FingerprintSet"
        if isinstance(bits, (Fingerprints, FingerprintSet)):
            bits = bits.bits
        rows = _pack_bits(what, bits)
        if rows.shape[0] < 1:
            raise ValueError(f"{what}: a set needs at least one row")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"{what} needs a CUDA (ROCm) device, got {self.device}: the MI355X HIP path has no CPU "
                               "fallback")
        self.bits = rows.to(self.device).contiguous()
        if self.bits.data_ptr() % 16:
            self.bits = self.bits.clone()
        self.n_bits = 32 * self.bits.shape[1]

    @classmethod
    def from_molecules(cls, nodes, edges, n_nodes, rules, *, radius: int = 2, n_bits: int = 2048):
        """The fingerprints of the given molecules as a set, built on the device (rows of malformed or empty molecules
        are all zero and are never anybody's neighbour)."""
        return cls(fingerprint(nodes, edges, n_nodes, rules, radius=radius, n_bits=n_bits).bits, device=nodes.device)

    def __len__(self):
        return self.bits.shape[0]


class SetComparison(_ResultBuffer):
    """What ``similarity`` / ``activity`` wrote, on the device: ``nearest`` / ``common`` / ``union`` [G] int32,
    ``max_sim`` [G] fp32 and, from ``activity``, ``decision`` / ``proba`` [G] fp32 (``None`` from ``similarity``);
    ``host()`` -> ``{name: numpy array}``."""

    def __init__(self, buf: torch.Tensor, G: int, scored: bool):
        super().__init__(buf, G, scored)
        if not scored:
            self.decision = self.proba = None

    @staticmethod
    @functools.lru_cache(maxsize=64)
    def layout(G: int, scored: bool) -> dict:
        return _pack(("nearest", "int32", (G,)), ("common", "int32", (G,)), ("union", "int32", (G,)),
                     ("max_sim", "float32", (G,)),
                     *([("decision", "float32", (G,)), ("proba", "float32", (G,))] if scored else []))

    @staticmethod
    def _host_result(a):
        return a


def _compare(what: str, fp, ref: FingerprintSet, weight, kind: int, gamma, intercept, prob_a, prob_b) -> SetComparison:
    if not isinstance(ref, FingerprintSet):
        raise TypeError(f"{what}: the set must be a FingerprintSet, got {type(ref).__name__}")
    query = fp.bits if isinstance(fp, (Fingerprints, FingerprintSet)) else fp
    if not isinstance(query, torch.Tensor) or query.dtype != torch.int32 or query.dim() != 2:
        raise TypeError(f"{what}: fp must be a Fingerprints, a FingerprintSet or a packed int32 tensor [G, n_bits / 32]")
    if not query.is_cuda:
        raise RuntimeError(f"{what} needs CUDA (ROCm) tensors (fp is on {query.device}): the MI355X HIP path has no CPU "
                           "fallback")
    if query.device != ref.bits.device:
        raise ValueError(f"{what}: fp is on {query.device}, the set on {ref.bits.device}")
    G, W = query.shape
    if W != ref.bits.shape[1]:
        raise ValueError(f"{what}: fp has {32 * W} bits, the set {ref.n_bits}")
    if not query.is_contiguous() or query.data_ptr() % 16:
        query = query.clone(memory_format=torch.contiguous_format)
    dev = query.device
    res = SetComparison.empty(dev, G, weight is not None)
    if G > 0:
        out = res._ptrs()
        with torch.cuda.device(dev):
            L.check(L.load().gi_fp_compare(
                G, len(ref), W, ref.bits.shape[1], query.data_ptr(), ref.bits.data_ptr(),
                None if weight is None else weight.data_ptr(), kind, gamma, intercept, prob_a, prob_b, out["nearest"],
                out["common"], out["union"], out["max_sim"], out.get("decision"), out.get("proba"),
                torch.cuda.current_stream(dev).cuda_stream), "gi_fp_compare")
    return res


def similarity(fp, ref: FingerprintSet) -> SetComparison:
    """Every fingerprint's nearest neighbour in a stored set, by Tanimoto, in one launch (``gi_fp_compare``) with no
    read-back.  ``fp``: ``fingerprint``'s result, a ``FingerprintSet`` or a packed int32 device tensor [G, n_bits / 32].
    ``nearest`` [G]: the set row of the largest ``c / u`` (c the common bits, u the union; decided in integers, ties to
    the lowest row), -1 for an all-zero fingerprint; ``common`` / ``union`` its c and u; ``max_sim`` = c / u in fp32."""
    return _compare("similarity", fp, ref, None, L.FP_TANIMOTO, 0.0, 0.0, 0.0, 0.0)


class KernelModel:
    """A two-class kernel model over fingerprints (a support vector classifier): ``decision(q) = intercept + sum_s
    dual_coef[s] K(q, support[s])`` with ``K`` = Tanimoto (``"tanimoto"``), ``exp(-gamma |q - s|**2)`` (``"rbf"``,
    needs ``gamma``) or the common bits (``"linear"``), and ``proba = 1 / (1 + exp(prob_a decision + prob_b))``
    (without ``prob_a`` / ``prob_b``: the plain logistic ``1 / (1 + exp(-decision))``).  **It must have been trained on
    ``fingerprint``'s rows, not on RDKit's.**"""

    def __init__(self, support: FingerprintSet, dual_coef, intercept: float, kind: str = "tanimoto", gamma=None,
                 prob_a=None, prob_b=None):
        what = "KernelModel"
        if not isinstance(support, FingerprintSet):
            raise TypeError(f"{what}: support must be a FingerprintSet, got {type(support).__name__}")
        if kind not in _FP_KINDS:
            raise ValueError(f"{what}: kind must be one of {sorted(_FP_KINDS)}, got {kind!r}")
        if kind == "rbf" and gamma is None:
            raise ValueError(f"{what}: the rbf kernel needs gamma")
        if (prob_a is None) != (prob_b is None):
            raise ValueError(f"{what}: give both prob_a and prob_b, or neither")
        coef = torch.as_tensor(np.asarray(dual_coef, dtype=np.float64).reshape(-1), dtype=torch.float32)
        if coef.numel() != len(support):
            raise ValueError(f"{what}: {coef.numel()} coefficients for {len(support)} support rows")
        self.support, self.kind, self.kind_code = support, kind, _FP_KINDS[kind]
        self.dual_coef = coef.to(support.device)
        self.intercept, self.gamma = float(intercept), 0.0 if gamma is None else float(gamma)
        self.prob_a, self.prob_b = (-1.0, 0.0) if prob_a is None else (float(prob_a), float(prob_b))

    @classmethod
    def from_sklearn(cls, svc, support_bits=None, device="cuda"):
        """From a fitted two-class ``sklearn.svm.SVC``, read by attribute (scikit-learn is never imported here).
        ``kernel="rbf"`` / ``"linear"``: the support rows are ``svc.support_vectors_`` (0 / 1).  ``kernel="precomputed"``
        is taken as a Tanimoto Gram matrix; ``support_bits`` must then hold the TRAINING fingerprints (rows
        ``svc.support_`` of it are the support).  With ``probability=True`` the Platt parameters are taken as
        ``prob_a = probA_``, ``prob_b = -probB_`` — the convention that reproduces ``predict_proba[:, 1]``
        (tests/golden/make_golden_fingerprint.py asserts it) up to libsvm's own iteration tolerance: for two classes
        libsvm does not return the Platt sigmoid itself but passes it through an iteration that stops at 0.0025, so
        ``predict_proba`` differs from the sigmoid of ``decision_function`` by up to a few 1e-3."""
        what = "KernelModel.from_sklearn"
        coef = np.asarray(svc.dual_coef_, dtype=np.float64)
        if coef.ndim != 2 or coef.shape[0] != 1:
            raise ValueError(f"{what}: a two-class model is needed (dual_coef_ has shape {coef.shape})")
        kernel = svc.kernel
        if kernel == "precomputed":
            if support_bits is None:
                raise ValueError(f"{what}: a precomputed (Tanimoto) kernel needs support_bits, the training fingerprints")
            rows = support_bits.bits if isinstance(support_bits, (Fingerprints, FingerprintSet)) else support_bits
            rows = _pack_bits(what, rows)
            rows = rows[torch.as_tensor(np.asarray(svc.support_, dtype=np.int64)).to(rows.device)]
            kind, gamma = "tanimoto", None
        elif kernel in ("rbf", "linear"):
            rows, kind = np.asarray(svc.support_vectors_), kernel
            gamma = float(svc._gamma) if kernel == "rbf" else None
            if rows.dtype == np.int32:                       # a dense 0 / 1 matrix, whatever its dtype
                rows = rows.astype(np.int8)
        else:
            raise ValueError(f"{what}: kernel {kernel!r} is not one of rbf, linear, precomputed")
        pa, pb = np.asarray(svc.probA_).reshape(-1), np.asarray(svc.probB_).reshape(-1)
        has = pa.size == 1 and pb.size == 1
        return cls(FingerprintSet(rows, device=device), coef[0], float(np.asarray(svc.intercept_).reshape(-1)[0]), kind,
                   gamma=gamma, prob_a=float(pa[0]) if has else None, prob_b=-float(pb[0]) if has else None)


def activity(fp, model: KernelModel) -> SetComparison:
    """The reference's ``ScoringFunction.compute_activity`` (ScoringFunction.py:162-192: a fingerprint and a
    ``predict_proba`` per molecule on the host) for the whole batch in one launch (``gi_fp_compare``), no read-back:
    ``proba`` [G] fp32 stands in for its result — **for a model trained on ``fingerprint``'s rows; these are not RDKit's
    ECFP bits**.  ``proba`` is 0 for an all-zero fingerprint (an empty or malformed molecule: the reference's
    ``except: pass``).  ``decision`` [G] is the fp32 kernel sum, made in a fixed order (equal inputs, equal bits);
    ``nearest`` / ``max_sim`` / ``common`` / ``union`` refer to the model's support rows."""
    if not isinstance(model, KernelModel):
        raise TypeError(f"activity: model must be a KernelModel, got {type(model).__name__}")
    return _compare("activity", fp, model.support, model.dual_coef, model.kind_code, model.gamma, model.intercept,
                    model.prob_a, model.prob_b)


def internal_diversity(fp) -> torch.Tensor:
    """One minus the mean Tanimoto similarity over the ordered pairs i != j of the non-empty fingerprints of a batch: a
    0-d fp32 device tensor, nothing read back (0 with fewer than two non-empty rows).  One ``gi_fp_compare`` launch of
    the batch against itself with unit weights."""
    what = "internal_diversity"
    own = fp
    if not isinstance(fp, FingerprintSet):
        rows = fp.bits if isinstance(fp, Fingerprints) else fp
        if not isinstance(rows, torch.Tensor):
            raise TypeError(f"{what}: fp must be a Fingerprints, a FingerprintSet or a packed int32 tensor")
        own = FingerprintSet(rows, device=rows.device)
    ones = torch.ones(len(own), dtype=torch.float32, device=own.bits.device)
    res = _compare(what, own, own, ones, L.FP_TANIMOTO, 0.0, 0.0, 0.0, 0.0)
    live = (res.nearest >= 0).to(torch.float32)
    m = live.sum()
    total = (res.decision * live).sum() - m                  # every non-empty row meets itself once, at 1
    return torch.where(m > 1, 1.0 - total / (m * (m - 1.0)).clamp_min(1.0), torch.zeros_like(m))


def target_size_score(n_nodes: torch.Tensor, target: int, max_n_nodes: int) -> torch.Tensor:
    """The reference's ``"target_size<k>"`` score component (ScoringFunction.py:111-129) from the ``n_nodes`` tensor:
    ``1 - |n - target| / (max_n_nodes - target)``, fp32, plain torch on ``n_nodes``' device, no read-back.  The
    reference's assertions become ``ValueError``; its division by zero at ``target == max_n_nodes`` is kept."""
    target, max_n_nodes = int(target), int(max_n_nodes)
    if not 0 < target <= max_n_nodes:
        raise ValueError(f"target_size_score: target {target} must be in (0, max_n_nodes = {max_n_nodes}]")
    n = n_nodes.to(torch.float32)
    size = target * torch.ones_like(n)
    return torch.ones_like(n) - torch.abs(n - size) / (max_n_nodes - size)


def compute_score(contributions: Sequence[torch.Tensor], *, score_type: str, thresholds: Sequence[float],
                  uniqueness: torch.Tensor, validity: torch.Tensor, termination: torch.Tensor) -> torch.Tensor:
    """The reference's ``ScoringFunction.compute_score`` (ScoringFunction.py:58-91) over ready-made contributions
    (``target_size_score``, ``activity(...).proba``, ...): plain torch on the tensors' device, no read-back, the
    caller's tensors left untouched.  The reference's quirks are kept: a single component IGNORES ``score_type``;
    ``"continuous"`` multiplies the components; ``"binary"`` multiplies the masks ``component > threshold`` (strict);
    the uniqueness, validity and termination masks multiply last."""
    contributions = list(contributions)
    if not contributions:
        raise ValueError("compute_score: at least one contribution is needed")
    if len(thresholds) != len(contributions):
        raise ValueError("compute_score: `contributions` and `thresholds` do not match")
    if len(contributions) == 1:
        final = contributions[0].clone()
    elif score_type == "continuous":
        final = contributions[0].clone()
        for component in contributions[1:]:
            final *= component
    elif score_type == "binary":
        masks = [(c > thresholds[k]).to(torch.uint8) for k, c in enumerate(contributions)]
        final = masks[0]
        for mask in masks[1:]:
            final *= mask
            final = final.float()
    else:
        raise NotImplementedError(f"compute_score: score_type {score_type!r}")
    final = final * uniqueness
    final = final * validity
    return final * termination


# ---- molecule strings ------------------------------------------------------------------------------------------------
#: status bits of ``smiles`` beyond the malformed bits of ``VALIDITY_STATUS_MESSAGES``
SMILES_STATUS_MESSAGES = {
    **{bit: VALIDITY_STATUS_MESSAGES[bit] for bit in (L.MOL_ONEHOT, L.MOL_BOND_PAST_N, L.MOL_VALUE, L.MOL_MULTI_BOND,
                                                      L.MOL_ASYMMETRIC, L.MOL_NODE_PAST_N)},
    L.SMI_EMPTY: "the molecule has no atoms: no string",
    L.SMI_SELF_LOOP: "an atom is bonded to itself: no string",
    L.SMI_OVER: "an atom has more bonds than any allowed valence of its element and charge (informational: the string "
                "is written)",
    L.SMI_FRAGMENTS: "more than one connected component, joined by '.' (informational)",
    L.SMI_AROMATIC: "a bond of order 1.5 is present: nothing is kekulised, no string (route the molecule to RDKit)",
    L.SMI_RING_LIMIT: "more than 99 ring bonds are open at once: no string",
    L.SMI_TRUNCATED: "the string needs more than max_len bytes: no string, length holds the need",
}
#: the bits that leave the text empty
NO_STRING_BITS = MALFORMED_BITS | L.SMI_EMPTY | L.SMI_SELF_LOOP | L.SMI_AROMATIC | L.SMI_RING_LIMIT | L.SMI_TRUNCATED


def default_smiles_len(N: int) -> int:
    """``smiles``' default ``max_len``: 12 N + 4 rounded up to a multiple of 16 (a default, not a bound: see
    ``gi_mol_smiles`` in include/graphinvent_amd.h)."""
    return (12 * int(N) + 4 + 15) // 16 * 16


class MoleculeStrings(_ResultBuffer):
    """What ``smiles`` wrote, on the device: ``text`` [G, max_len] uint8 (zero padded), ``length`` / ``status`` [G]
    int32, ``atom_pos`` [G, N] int32 (the byte offset of every atom's token; -1 past n and throughout a molecule whose
    text is empty); ``host()`` -> ``(list of str, length, status, atom_pos)`` with one copy and one synchronisation."""

    def __init__(self, buf: torch.Tensor, G: int, N: int, max_len: int):
        super().__init__(buf, G, N, max_len)
        self.N, self.max_len = N, max_len

    @staticmethod
    @functools.lru_cache(maxsize=64)
    def layout(G: int, N: int, max_len: int) -> dict:
        return _pack(("text", "uint8", (G, max_len)), ("length", "int32", (G,)), ("status", "int32", (G,)),
                     ("atom_pos", "int32", (G, N)))

    @staticmethod
    def _host_result(a):
        text, length, status = a["text"], a["length"], a["status"]
        rows = text.tobytes()
        width = text.shape[1]
        strings = ["" if int(status[g]) & NO_STRING_BITS else rows[g * width:g * width + int(length[g])].decode("ascii")
                   for g in range(text.shape[0])]
        return strings, length, status, a["atom_pos"]


def symbol_table(atom_types: Sequence[str]) -> np.ndarray:
    """The element symbols as the [A, 2] byte table ``gi_mol_smiles`` reads (the second byte 0 for a one-letter
    symbol); ``ValueError`` for a symbol that is not one or two ASCII letters."""
    sym = np.zeros((len(atom_types), 2), np.uint8)
    for a, s in enumerate(atom_types):
        if not (isinstance(s, str) and 1 <= len(s) <= 2 and s.isascii() and s.isalpha()):
            raise ValueError(f"smiles: the element symbol {s!r} is not one or two ASCII letters")
        sym[a, :len(s)] = np.frombuffer(s.encode("ascii"), np.uint8)
    return sym


def _smiles_tables(what: str, rules: ValenceRules):
    """-> (symbols [A, 2] uint8, charges [C] int8) on the rules' device, uploaded once per rules."""
    tables = rules.__dict__.get("_smiles")
    if tables is None:
        if rules.device is None:
            raise RuntimeError(f"{what}: the rules were built with device=None and hold no device tables (no CPU "
                               "fallback)")
        tables = rules.__dict__["_smiles"] = (torch.from_numpy(symbol_table(rules.atom_types)).to(rules.device),
                                              torch.tensor(rules.formal_charge, dtype=torch.int8, device=rules.device))
    return tables


_canonical = canonical                                      # ``smiles`` has a keyword of that name


def smiles(nodes: torch.Tensor, edges: torch.Tensor, n_nodes: Optional[torch.Tensor], rules: ValenceRules, *,
           rank: Optional[torch.Tensor] = None, canonical: bool = False, hydrogens: Optional[str] = None,
           max_len: Optional[int] = None) -> MoleculeStrings:
    """Every molecule as a SMILES string — what the reference's ``util.write_graphs_to_smi`` (util.py:520-585) gets from
    one ``RWMol``, one ``SanitizeMol`` and one ``MolToSmiles`` per molecule on the host — for all G molecules in one
    launch (``gi_mol_smiles``), with no RDKit and no read-back; inputs as ``validity``.

    **THE STRING IS A FAITHFUL SPELLING OF THE LABELLED GRAPH, NOT RDKit's CANONICAL SMILES**: an OpenSMILES subset with
    no aromaticity (nothing is perceived, nothing is kekulised: a bond of order 1.5 gives ``SMI_AROMATIC`` and no
    string, so that the caller can route such molecules to RDKit), no stereo marks (the reference's ``graph_to_mol``
    sets no chiral tag either, only the ``_CIPCode`` property, so its strings carry none), and hydrogen counts that are
    ``rules``' fill or the stored ones.  Any OpenSMILES reader gets the labelled graph back (tests/smiles_model.py
    holds one, and the Python specification of the writer; include/graphinvent_amd.h has the grammar).

    ``rank`` [G, N] int32 on the device: the traversal key of every atom (ties go to the lower index; without it the key
    is the input index).  Components come in ascending order of their lowest-key atom, each walked depth-first from it
    with the neighbours in ascending key.  ``canonical=True`` calls ``canonical`` and passes its ``rank`` (one launch
    more, no read-back; giving both is a ``ValueError``): then two molecules get the same string exactly when
    ``canonical`` gives them the same form — that includes its documented incompleteness on graphs whose refinement
    cells are not orbits — whereas the reference compares RDKit's canonical SMILES.

    ``hydrogens``: ``"fill"`` — ``validity``'s ``h = v* - x``, 0 for an atom over its valence — or ``"stored"`` — the
    count in the implicit-H segment, the reference's ``_TotalNumHs`` (needs ``rules.imp_H``); default ``"stored"`` when
    the rules have such a segment.  An atom is written bare (``C``) when its symbol is in the organic subset, it has
    no charge and its count equals the OpenSMILES implicit count, else in brackets (``[NH4+]``).  The symbols are
    ``rules.atom_types``: one or two ASCII letters each, else ``ValueError``.

    ``max_len`` (a multiple of 16, at most ``lib.SMI_MAX_LEN``) defaults to ``default_smiles_len(N)``: enough for
    molecules but not a bound, a dense graph needs more and gets ``SMI_TRUNCATED`` with the need in ``length``.

    Result (``MoleculeStrings``, views of one device buffer): ``text`` [G, max_len] uint8, ``length``, ``status`` [G]
    int32 (``SMILES_STATUS_MESSAGES``: the malformed bits of ``validity``, ``SMI_EMPTY``, ``SMI_SELF_LOOP``,
    ``SMI_AROMATIC``, ``SMI_RING_LIMIT`` — empty text, length 0 — ``SMI_TRUNCATED`` — empty text, length = the need —
    and the informational ``SMI_OVER`` and ``SMI_FRAGMENTS``), ``atom_pos`` [G, N] int32.  ``.host()`` is one copy and
    one synchronisation.  G = 0 is answered without a launch."""
    what = "smiles"
    A, Cn, H = _rules_groups(what, rules)
    if canonical and rank is not None:
        raise ValueError(f"{what}: give rank or canonical=True, not both")
    if hydrogens is None:
        hydrogens = "stored" if H else "fill"
    if hydrogens not in ("fill", "stored"):
        raise ValueError(f"{what}: hydrogens must be 'fill' or 'stored', got {hydrogens!r}")
    if hydrogens == "stored" and not H:
        raise ValueError(f"{what}: hydrogens='stored' needs rules with an implicit-H segment (imp_H)")
    symbol_table(rules.atom_types)                           # raises for a symbol that cannot be written
    if not all(-127 <= c <= 127 for c in rules.formal_charge):
        raise ValueError(f"{what}: formal charges {rules.formal_charge} must lie in [-127, 127]")
    G, N, Fn, Fe, dtype, n_nodes, nn_bytes, _ = _check_inputs(what, nodes, edges, n_nodes, None, False)
    max_len = default_smiles_len(N) if max_len is None else max_len
    if (not isinstance(max_len, (int, np.integer)) or isinstance(max_len, bool) or max_len % 16
            or not 16 <= max_len <= L.SMI_MAX_LEN):
        raise ValueError(f"{what}: max_len must be a multiple of 16 in [16, {L.SMI_MAX_LEN}], got {max_len!r}")
    max_len = int(max_len)
    dev = nodes.device
    A, Cn, H, order2 = _check_rules(what, rules, Fn, Fe, dev)
    symbols, charges = _smiles_tables(what, rules)
    if rank is not None:
        if not isinstance(rank, torch.Tensor) or not rank.is_cuda or rank.device != dev:
            raise RuntimeError(f"{what}: rank must be a CUDA tensor on {dev} (no CPU fallback)")
        if tuple(rank.shape) != (G, N) or rank.dtype != torch.int32 or not rank.is_contiguous():
            raise ValueError(f"{what}: rank must be a contiguous int32 tensor of shape ({G}, {N}), got {rank.dtype} "
                             f"{tuple(rank.shape)}")
    elif canonical:
        rank = _canonical(nodes, edges, n_nodes).rank
    res = MoleculeStrings.empty(dev, G, N, max_len)
    if G > 0:
        out = res._ptrs()
        with torch.cuda.device(dev):
            L.check(L.load().gi_mol_smiles(
                G, N, Fn, Fe, nodes.data_ptr(), edges.data_ptr(), dtype,
                None if n_nodes is None else n_nodes.data_ptr(), nn_bytes, A, Cn, H, rules.allowed_mask.data_ptr(),
                order2.data_ptr(), None if rules.h_values is None else rules.h_values.data_ptr(), charges.data_ptr(),
                symbols.data_ptr(), int(hydrogens == "stored"), None if rank is None else rank.data_ptr(), max_len,
                out["text"], out["length"], out["status"], out["atom_pos"],
                torch.cuda.current_stream(dev).cuda_stream), "gi_mol_smiles")
    return res


def write_smi(path, strings, *, valid=None, placeholder: str = "[Xe]") -> int:
    """Write a ``.smi`` file in the layout of the reference's shipped ones (``SmilesWriter``'s): the header row
    ``SMILES Name``, then one ``<string> <row index>`` row per molecule.  ``strings``: ``smiles``' result (read back
    here, with its one copy) or a sequence of str.  ``valid`` [G] (a tensor, e.g. ``validity(...).valid``, or a
    sequence; non-zero = valid; default all): a molecule whose entry is 0, and one whose string is empty, is written as
    ``placeholder`` — the reference's ``[Xe]`` line for a molecule that fails sanitisation (util.py:573-578).  Returns
    the number of placeholder rows."""
    rows = strings.host()[0] if isinstance(strings, MoleculeStrings) else list(strings)
    if valid is None:
        ok = [True] * len(rows)
    else:
        if isinstance(valid, torch.Tensor) and valid.is_cuda:
            with _host_sync_allowed():                       # the file needs the values: one read-back
                valid = valid.detach().cpu()
        if isinstance(valid, torch.Tensor):
            valid = valid.detach().numpy()
        ok = [bool(v) for v in np.asarray(valid).reshape(-1)]
        if len(ok) != len(rows):
            raise ValueError(f"write_smi: {len(rows)} strings but {len(ok)} validity entries")
    if not placeholder or any(ch.isspace() for ch in placeholder):
        raise ValueError(f"write_smi: placeholder {placeholder!r} must be a non-empty string without blanks")
    replaced = 0
    with open(path, "w") as f:
        f.write("SMILES Name\n")
        for k, s in enumerate(rows):
            if not s or not ok[k]:
                s, replaced = placeholder, replaced + 1
            f.write(f"{s} {k}\n")
    return replaced


# ---- molecule reading ------------------------------------------------------------------------------------------------
#: status bits of ``read_smiles`` (``lib.SMR_*``); every bit of ``lib.SMR_ERROR`` leaves the all-zero molecule
READ_STATUS_MESSAGES = {
    L.SMR_MULTI_BOND: "the same pair of atoms is bonded twice",
    L.SMR_EMPTY: "the string is empty",
    L.SMR_SELF_LOOP: "a ring closes on the atom that opened it",
    L.SMR_OVER: "an atom has more bonds than any allowed valence of its element and charge (informational: the "
                "molecule is written)",
    L.SMR_FRAGMENTS: "more than one connected component (informational)",
    L.SMR_AROMATIC: "a lowercase (aromatic) atom or ':': nothing is kekulised, no molecule (route the string to RDKit)",
    L.SMR_TOO_MANY: "more atoms than max_n_nodes: no molecule, n_nodes holds the need",
    L.SMR_SYNTAX: "not a string of the grammar (an unclosed bracket or branch, a dangling bond, a bond or ring digit "
                  "without an atom, '..', an unknown byte, '%' without two digits, bare H, a length outside the row)",
    L.SMR_RING_OPEN: "a ring number is left open",
    L.SMR_RING_ORDER: "the two ends of a ring bond state different bond orders",
    L.SMR_ELEMENT: "an element that is not in the rules' atom types",
    L.SMR_CHARGE: "a formal charge that is not in the rules' charges",
    L.SMR_HCOUNT: "a hydrogen count that is not in the rules' implicit-H values",
    L.SMR_BOND_ORDER: "a bond order that the rules' bond types do not hold",
    L.SMR_STEREO: "a stereo mark ('@', '/', '\\'): no molecule (stereo='drop' skips the marks; or route the string to "
                  "RDKit)",
    L.SMR_STEREO_DROPPED: "stereo marks were skipped (informational)",
    L.SMR_UNSUPPORTED: "an isotope, an atom class, '++' / '--', '$' or the wildcard",
}


#: the two bits ``read_smiles(..., aromatic="kekulize")`` adds (``lib.SMR_KEKULE`` is an error bit: ``lib.SMR_READ_ERROR``)
KEKULE_STATUS_MESSAGES = {
    L.SMR_KEKULE: "the aromatic atoms have no Kekule structure (no perfect matching of the atoms that need a double "
                  "bond): no molecule",
    L.SMR_KEKULIZED: "aromatic atoms were read and kekulised by the library's own rule (informational)",
}


def describe_read_status(bits: int) -> str:
    return "; ".join(msg for table in (READ_STATUS_MESSAGES, KEKULE_STATUS_MESSAGES) for bit, msg in table.items()
                     if bits & bit) or "read"


def pack_strings(strings, max_len: Optional[int] = None, device="cuda"):
    """Python strings (or ``bytes``) as the byte rows ``read_smiles`` takes — ``smiles``' own layout — built in ONE host
    buffer and uploaded with ONE copy: ``(text [G, max_len] uint8 zero padded, length [G] int32)``, views of one device
    buffer.  ``max_len`` (a multiple of 16, at most ``lib.SMI_MAX_LEN``) defaults to the longest string rounded up; a
    string that is longer, or not ASCII, is a ``ValueError`` that names its row."""
    raw = []
    for g, s in enumerate(strings):
        if isinstance(s, str):
            try:
                s = s.encode("ascii")
            except UnicodeEncodeError:
                raise ValueError(f"pack_strings: string {g} ({s!r}) is not ASCII") from None
        elif not isinstance(s, (bytes, bytearray)):
            raise TypeError(f"pack_strings: string {g} is a {type(s).__name__}, expected str or bytes")
        raw.append(bytes(s))
    need = max([len(r) for r in raw] + [1])
    if max_len is None:
        max_len = (need + 15) // 16 * 16
    if (not isinstance(max_len, (int, np.integer)) or isinstance(max_len, bool) or max_len % 16
            or not 16 <= max_len <= L.SMI_MAX_LEN):
        raise ValueError(f"pack_strings: max_len must be a multiple of 16 in [16, {L.SMI_MAX_LEN}], got {max_len!r} "
                         f"(the longest string has {need} bytes)")
    max_len, G = int(max_len), len(raw)
    if need > max_len:
        g = next(g for g, r in enumerate(raw) if len(r) > max_len)
        raise ValueError(f"pack_strings: string {g} has {len(raw[g])} bytes, max_len is {max_len}")
    host = np.zeros(G * max_len + 4 * G, np.uint8)
    host[:G * max_len] = np.frombuffer(b"".join([r.ljust(max_len, b"\0") for r in raw]), np.uint8)
    host[G * max_len:].view(np.int32)[:] = np.fromiter(map(len, raw), np.int32, count=G)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"pack_strings needs a CUDA (ROCm) device, got {dev}: the MI355X HIP path has no CPU fallback")
    with _host_sync_allowed():                               # (set-up: a host buffer's upload may synchronise)
        buf = torch.from_numpy(host).to(dev)
    if G == 0:                                               # (an empty slice has no stride to view as int32)
        return buf.view(0, max_len), torch.empty(0, dtype=torch.int32, device=dev)
    return buf[:G * max_len].view(G, max_len), buf[G * max_len:].view(torch.int32)


class ReadMolecules(_ResultBuffer):
    """What ``read_smiles`` read, on the device: ``nodes`` [G, N, Fn] / ``edges`` [G, N, N, Fe] int8 (what
    ``routes.RouteLoader``, ``SeedBank``, ``SeenSet.add``, ``FingerprintSet.from_molecules`` and
    ``likelihood.molecule_log_likelihood`` take), ``n_nodes`` / ``status`` [G] int32, ``atom_pos`` [G, N] int32 (the byte
    offset of every atom's token, -1 past n); ``host()`` -> ``(nodes, edges, n_nodes, status, atom_pos)`` with one copy
    and one synchronisation."""

    def __init__(self, buf: torch.Tensor, G: int, N: int, Fn: int, Fe: int):
        super().__init__(buf, G, N, Fn, Fe)
        self.N, self.Fn, self.Fe = N, Fn, Fe

    @staticmethod
    @functools.lru_cache(maxsize=64)
    def layout(G: int, N: int, Fn: int, Fe: int) -> dict:
        return _pack(("atom_pos", "int32", (G, N)), ("n_nodes", "int32", (G,)), ("status", "int32", (G,)),
                     ("_pad", "uint8", (-4 * G * (N + 2) % 16,)),                # the molecule rows start a 16-byte piece
                     ("nodes", "int8", (G, N, Fn)), ("edges", "int8", (G, N, N, Fe)))

    @staticmethod
    def _host_result(a):
        return a["nodes"], a["edges"], a["n_nodes"], a["status"], a["atom_pos"]


def read_smiles(strings, rules: ValenceRules, max_n_nodes: int, *, length: Optional[torch.Tensor] = None,
                n_chirality: int = 0, none_chirality: int = 0, stereo: str = "error",
                n_bond_types: Optional[int] = None, aromatic: str = "error") -> ReadMolecules:
    """SMILES strings into int8 molecules — what the reference's preprocessing gets from one ``MolFromSmiles`` and one
    graph construction per molecule on the host — for all G strings in one launch (``gi_smiles_read``), with no RDKit
    and no read-back.  The exact inverse of ``smiles`` on what ``smiles`` writes: ``read_smiles(smiles(m))`` is ``m``
    with its atoms in the order of the string (``argsort(atom_pos)``), byte for byte.

    **WHAT IT IS NOT**: by default no aromatic input (``c1ccccc1``) and no stereo (``@``, ``/``, ``\\``).
    Such a string gets ``SMR_AROMATIC`` / ``SMR_STEREO`` and no molecule, so that the caller can route it to RDKit;
    ``stereo="drop"`` skips the marks instead (``SMR_STEREO_DROPPED``).  Atoms are numbered IN STRING ORDER, which is
    not the order of the reference's preprocessing: train with ``routes.RouteLoader(reorder=...)``.  The grammar is in
    include/graphinvent_amd.h at ``gi_smiles_read``; tests/smiles_read_model.py is the Python specification.

    ``aromatic="kekulize"`` (``gi_smiles_read_arom``) reads aromatic atoms (``b c n o p s``, ``[nH]``, ``[se]`` ...) and
    ``:`` and assigns single and double bonds to the aromatic-marked bonds inside the same launch: a perfect matching
    of the atoms that need a double bond, chosen deterministically.  **IT IS NOT RDKit'S KEKULISATION**: no ring or
    aromaticity perception and no canonical choice, so two strings of one compound can come out as two different Kekule
    structures, which ``unique`` counts as two molecules.  A string without a Kekule structure gets ``SMR_KEKULE`` (in
    ``lib.SMR_READ_ERROR``) and no molecule; one that had aromatic atoms and was read gets ``SMR_KEKULIZED``.  The rule
    is written out at ``gi_smiles_read_arom`` in the header; tests/kekule_read_model.py is its specification.  Writing
    aromatic SMILES, stereo and order-1.5 bonds (``use_aromatic_bonds``) stay out of scope.

    ``strings``: a sequence of ``str`` (packed by ``pack_strings``: one host buffer, one copy), ``smiles``' result, or a
    [G, max_len] uint8 tensor on the device (16-byte aligned, max_len a multiple of 16) with ``length`` [G] int32 or
    without (a string then ends at its first zero byte).  A node row is ``rules``' segments type | charge | implicit H,
    then ``n_chirality`` entries of which ``none_chirality`` is set; a bare atom's hydrogens are the OpenSMILES implicit
    count, a bracket atom's the stated ones, stored only when the rules have an implicit-H segment.  ``n_bond_types``:
    Fe, default the rules' bond orders or 3.

    Result (``ReadMolecules``, views of one device buffer): ``nodes``, ``edges``, ``n_nodes``, ``status``
    (``READ_STATUS_MESSAGES``, ``KEKULE_STATUS_MESSAGES``; any bit of ``lib.SMR_ERROR``, or of ``lib.SMR_READ_ERROR``
    with ``aromatic="kekulize"``, leaves the all-zero molecule, which the rest of the library treats as empty, and
    ``SMR_TOO_MANY`` leaves the atoms needed in ``n_nodes``), ``atom_pos``.  G = 0 is answered without a launch."""
    what = "read_smiles"
    A, Cn, H = _rules_groups(what, rules)
    if stereo not in ("error", "drop"):
        raise ValueError(f"{what}: stereo must be 'error' or 'drop', got {stereo!r}")
    if aromatic not in ("error", "kekulize"):
        raise ValueError(f"{what}: aromatic must be 'error' or 'kekulize', got {aromatic!r}")
    for name, v, lo in (("max_n_nodes", max_n_nodes, 1), ("n_chirality", n_chirality, 0),
                        ("none_chirality", none_chirality, 0)):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or v < lo:
            raise ValueError(f"{what}: {name} must be an integer >= {lo}, got {v!r}")
    N, Fn = int(max_n_nodes), A + Cn + H + int(n_chirality)
    if n_chirality and none_chirality >= n_chirality:
        raise ValueError(f"{what}: none_chirality {none_chirality} is outside the {n_chirality} chirality entries")
    Fe = (len(rules.bond_orders) if rules.bond_orders is not None else 3) if n_bond_types is None else int(n_bond_types)
    if N > L.GI_MAX_NODES or not 1 <= Fe <= L.GI_MAX_GROUPS or Fn > L.ANALYZE_MAX_FN:
        raise ValueError(f"{what}: needs max_n_nodes <= {L.GI_MAX_NODES}, 1 <= Fe <= {L.GI_MAX_GROUPS}, Fn <= "
                         f"{L.ANALYZE_MAX_FN}; got N {N}, Fn {Fn}, Fe {Fe}")
    symbol_table(rules.atom_types)                           # raises for a symbol that cannot be spelt
    if not all(-127 <= c <= 127 for c in rules.formal_charge):
        raise ValueError(f"{what}: formal charges {rules.formal_charge} must lie in [-127, 127]")
    A, Cn, H, order2 = _check_rules(what, rules, Fn, Fe, None)    # the text's device is known only below
    if isinstance(strings, MoleculeStrings):
        if length is not None:
            raise ValueError(f"{what}: smiles' result brings its own length")
        text, length = strings.text, strings.length
    elif isinstance(strings, torch.Tensor):
        text = strings
    else:
        if length is not None:
            raise ValueError(f"{what}: length goes with a byte tensor, a list of strings brings its own")
        text, length = pack_strings(strings, device=rules.device)
    if not text.is_cuda:
        raise RuntimeError(f"{what} needs CUDA (ROCm) tensors (the text is on {text.device}): the MI355X HIP path has no "
                           "CPU fallback")
    if text.dim() != 2 or text.dtype != torch.uint8 or not text.is_contiguous():
        raise ValueError(f"{what}: the text must be a contiguous [G, max_len] uint8 tensor, got {text.dtype} "
                         f"{tuple(text.shape)}")
    G, max_len = text.shape
    if max_len % 16 or not 16 <= max_len <= L.SMI_MAX_LEN or text.data_ptr() % 16:
        raise ValueError(f"{what}: max_len must be a multiple of 16 in [16, {L.SMI_MAX_LEN}] and the text 16-byte "
                         f"aligned, got max_len {max_len}")
    dev = text.device
    if length is not None:
        if not isinstance(length, torch.Tensor) or not length.is_cuda or length.device != dev:
            raise RuntimeError(f"{what}: length must be a CUDA tensor on {dev} (no CPU fallback)")
        if tuple(length.shape) != (G,) or length.dtype != torch.int32 or not length.is_contiguous():
            raise ValueError(f"{what}: length must be a contiguous int32 tensor of shape ({G},), got {length.dtype} "
                             f"{tuple(length.shape)}")
    symbols, charges = _smiles_tables(what, rules)
    if order2.device != dev:
        raise ValueError(f"{what}: the text is on {dev}, the rules' tables on {order2.device}")
    res = ReadMolecules.empty(dev, G, N, Fn, Fe)
    if G > 0:
        out = res._ptrs()
        head = (G, N, Fn, Fe, text.data_ptr(), None if length is None else length.data_ptr(), max_len, A, Cn, H,
                rules.allowed_mask.data_ptr(), order2.data_ptr(),
                None if rules.h_values is None else rules.h_values.data_ptr(), charges.data_ptr(), symbols.data_ptr(),
                int(none_chirality), int(stereo == "drop"))
        with torch.cuda.device(dev):
            tail = (out["nodes"], out["edges"], out["n_nodes"], out["status"], out["atom_pos"],
                    torch.cuda.current_stream(dev).cuda_stream)
            if aromatic == "kekulize":
                L.check(L.load().gi_smiles_read_arom(*head, 1, *tail), "gi_smiles_read_arom")
            else:
                L.check(L.load().gi_smiles_read(*head, *tail), "gi_smiles_read")
    return res


class SmiMolecules:
    """What ``read_smi`` read: ``nodes`` [G, N, Fn] / ``edges`` [G, N, N, Fe] int8, ``n_nodes`` / ``status`` [G] int32
    on the device, row for row the file's lines, and ``names`` (the second column, ``""`` without one) on the host."""

    def __init__(self, nodes, edges, n_nodes, status, names):
        self.nodes, self.edges, self.n_nodes, self.status, self.names = nodes, edges, n_nodes, status, names

    def __len__(self):
        return len(self.names)


def read_smi(path, rules: ValenceRules, max_n_nodes: int, *, batch: int = 8192, **kw) -> SmiMolecules:
    """The inverse of ``write_smi``: a ``.smi`` file into int8 molecules on the device, ``batch`` lines per
    ``read_smiles`` launch (``**kw`` goes to it), nothing read back.  A first line whose first column is ``SMILES`` is
    the header and is skipped; of every other line the first blank-separated column is the string and the second the
    name.  NO LINE IS LEFT OUT: a string with an error bit — ``write_smi``'s ``[Xe]`` placeholder under rules without
    Xe, an aromatic string, an empty line — stays in its row as the all-zero molecule with its ``status``; it is the
    caller who masks (``status & lib.SMR_ERROR``; ``lib.SMR_READ_ERROR`` with ``aromatic="kekulize"``, which goes
    through ``**kw`` like every other option) or routes such rows to RDKit."""
    if not isinstance(batch, (int, np.integer)) or isinstance(batch, bool) or batch < 1:
        raise ValueError(f"read_smi: batch must be a positive integer, got {batch!r}")
    with open(path, "rb") as f:
        lines = f.read().split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()                                          # the file ends with a newline, not with an empty line
    cols = [line.split() for line in lines]
    if cols and cols[0] and cols[0][0] == b"SMILES":
        cols = cols[1:]
    strings = [c[0] if c else b"" for c in cols]
    names = [c[1].decode("utf-8", "replace") if len(c) > 1 else "" for c in cols]
    parts = [read_smiles(strings[k:k + batch], rules, max_n_nodes, **kw) for k in range(0, len(strings), batch)]
    if not parts:
        parts = [read_smiles([], rules, max_n_nodes, **kw)]
    if len(parts) == 1:
        one = parts[0]
        return SmiMolecules(one.nodes, one.edges, one.n_nodes, one.status, names)
    return SmiMolecules(*(torch.cat([getattr(p, name) for p in parts]) for name in ("nodes", "edges", "n_nodes", "status")),
                        names)


# ---- substructure search ---------------------------------------------------------------------------------------------
#: status bits of ``substructure`` beyond the malformed bits of ``VALIDITY_STATUS_MESSAGES``
SUBSTRUCTURE_STATUS_MESSAGES = {
    **{bit: VALIDITY_STATUS_MESSAGES[bit] for bit in (L.MOL_ONEHOT, L.MOL_BOND_PAST_N, L.MOL_VALUE, L.MOL_MULTI_BOND,
                                                      L.MOL_ASYMMETRIC, L.MOL_NODE_PAST_N)},
    L.VAL_EMPTY: "the molecule has no atoms: it matches nothing",
    L.VAL_SELF_LOOP: "an atom is bonded to itself: the molecule matches nothing",
    L.SUB_STEP_LIMIT: "an anchor was given up after max_steps steps (counted in n_limited; it counts as no match)",
    L.SUB_PATTERN_INDEX: "pattern_index is outside [0, P): no match",
}
_SUB_HDR, _SUB_REC, _SUB_ROW = 8, 4, 8                       # words of the table's header, a record's and a row's head


def _sub_array(what: str, name: str, x, ndim: int) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    x = np.asarray(x)
    if x.ndim != ndim or x.dtype == object:
        raise ValueError(f"{what}: {name} must be a {ndim}-dimensional array, got shape {x.shape}")
    return x


class SubstructureSet:
    """P patterns for ``substructure``, validated, planned and packed ONCE (``table``, int32, on the host and on
    ``device``; the layout is in include/graphinvent_amd.h at ``gi_mol_substructure``).

    **A PATTERN IS NOT SMARTS**: a connected labelled graph of 1 to 32 atoms.  ``type_mask`` [P, Np_max, A] and
    ``charge_mask`` [P, Np_max, C]: per atom a 0 / 1 row over the atom types / formal charges of the rules the molecules
    are read with (all zero: any; several ones: any of these).  ``bond_mask`` [P, Np_max, Np_max, Fe], symmetric: per
    atom pair a 0 / 1 row over the bond types (all zero: no pattern bond; several ones: any of these).  ``degree`` /
    ``min_h`` [P, Np_max] (optional): the exact number of bonded partners / at least this many hydrogens by the rules'
    fill (``validity``'s ``atom_h``), -1: any.  Patterns of different sizes share the arrays: Np of a pattern is one past
    its last atom that has a bond or a predicate, at least 1; what lies behind is padding.  ``names``: P strings.

    An empty set, an atom on its own diagonal, an asymmetric ``bond_mask`` and a pattern that is not connected raise
    ``ValueError``.  ``order`` / ``parent`` / ``back`` hold every pattern's plan: its atoms in breadth-first order from
    atom 0 (neighbours ascending), every position's parent position and its other bonds to earlier positions.
    ``device=None`` keeps the host table only (``substructure`` refuses such a set)."""

    def __init__(self, type_mask, charge_mask, bond_mask, *, degree=None, min_h=None, names=None, device="cuda"):
        what = "SubstructureSet"
        tm, cm = _sub_array(what, "type_mask", type_mask, 3) != 0, _sub_array(what, "charge_mask", charge_mask, 3) != 0
        bm = _sub_array(what, "bond_mask", bond_mask, 4) != 0
        P, Npm, A = tm.shape
        if P < 1 or Npm < 1 or A < 1:
            raise ValueError(f"{what}: at least one pattern of at least one atom is needed, got type_mask {tm.shape}")
        if cm.shape[:2] != (P, Npm) or cm.shape[2] < 1 or bm.shape[:3] != (P, Npm, Npm) or bm.shape[3] < 1:
            raise ValueError(f"{what}: charge_mask {cm.shape} / bond_mask {bm.shape} do not match type_mask {tm.shape} "
                             "([P, Np, A], [P, Np, C], [P, Np, Np, Fe])")
        C_, Fe = cm.shape[2], bm.shape[3]
        if Npm > L.SUB_MAX_ATOMS or P > L.SUB_MAX_PATTERNS or Fe > L.GI_MAX_GROUPS or A + C_ > L.ANALYZE_MAX_FN:
            raise ValueError(f"{what}: at most {L.SUB_MAX_ATOMS} atoms per pattern, {L.SUB_MAX_PATTERNS} patterns, "
                             f"{L.GI_MAX_GROUPS} bond types and {L.ANALYZE_MAX_FN} node entries; got Np {Npm}, P {P}, "
                             f"Fe {Fe}, A + C {A + C_}")
        extra = []
        for name, x, hi in (("degree", degree, L.GI_MAX_NODES - 1), ("min_h", min_h, 15)):
            if x is None:
                x = np.full((P, Npm), -1, np.int64)
            else:
                x = _sub_array(what, name, x, 2)
                if x.shape != (P, Npm) or not np.issubdtype(x.dtype, np.integer) or x.min() < -1 or x.max() > hi:
                    raise ValueError(f"{what}: {name} must be integers in [-1, {hi}] of shape ({P}, {Npm})")
            extra.append(x.astype(np.int64))
        deg, mh = extra
        if names is not None and (len(names) != P or len(set(names)) != P):
            raise ValueError(f"{what}: names must be {P} different strings")
        self.names = None if names is None else [str(s) for s in names]
        if (bm != bm.transpose(0, 2, 1, 3)).any():
            raise ValueError(f"{what}: bond_mask must be symmetric in its two atom axes")
        if bm[:, np.arange(Npm), np.arange(Npm)].any():
            raise ValueError(f"{what}: bond_mask has an atom bonded to itself")
        bonded = bm.any(axis=3)
        marked = bonded.any(axis=2) | tm.any(axis=2) | cm.any(axis=2) | (deg >= 0) | (mh >= 0)
        self.n_atoms = [max(1, int(np.flatnonzero(marked[p])[-1]) + 1 if marked[p].any() else 1) for p in range(P)]
        self.order, self.parent, self.back = [], [], []
        for p in range(P):
            order, parent, back = self._plan(bonded[p], self.n_atoms[p], p if self.names is None else self.names[p])
            self.order.append(order), self.parent.append(parent), self.back.append(back)
        self.dims, self.Np_max = (A, C_, Fe), Npm
        TW, CW = (A + 31) // 32, (C_ + 31) // 32
        Bmax = -(-max(sum(len(b) for b in back) for back in self.back) // 4) * 4
        R = _SUB_ROW + -(-(TW + CW) // 4) * 4
        S = _SUB_REC + Npm * R + Bmax
        table = np.zeros(_SUB_HDR + P * S, np.int64)
        table[:_SUB_HDR] = [P, Npm, A, C_, Fe, TW, CW, Bmax]
        bits = lambda row, words, size: [sum(1 << int(b - 32 * w) for b in (np.flatnonzero(row) if row.any()
                                                                            else range(size)) if 32 * w <= b < 32 * w + 32)
                                         for w in range(words)]
        word = lambda row: sum(1 << int(t) for t in np.flatnonzero(row))
        for p in range(P):
            rec = _SUB_HDR + p * S
            table[rec] = self.n_atoms[p]
            n_back = 0
            for k, atom in enumerate(self.order[p]):
                row = rec + _SUB_REC + k * R
                par = self.parent[p][k]
                table[row:row + 8] = [par, word(bm[p, atom, self.order[p][par]]) if k else 0, n_back,
                                      len(self.back[p][k]), atom, deg[p, atom], mh[p, atom], 0]
                table[row + 8:row + 8 + TW] = bits(tm[p, atom], TW, A)
                table[row + 8 + TW:row + 8 + TW + CW] = bits(cm[p, atom], CW, C_)
                for q in self.back[p][k]:
                    table[rec + _SUB_REC + Npm * R + n_back] = q | (word(bm[p, atom, self.order[p][q]]) << 8)
                    n_back += 1
        self.table = (table & 0xffffffff).astype(np.uint32).view(np.int32)
        self.device = None if device is None else torch.device(device)
        self.table_dev = None
        if self.device is not None:
            if self.device.type != "cuda":
                raise RuntimeError(f"{what} needs a CUDA (ROCm) device, got {self.device}: the MI355X HIP path has no CPU "
                                   "fallback (device=None keeps the table on the host, for inspection only)")
            self.table_dev = torch.from_numpy(self.table).to(self.device)

    @staticmethod
    def _plan(bonded, Np: int, name):
        order, parent_atom, head = [0], {0: 0}, 0
        while head < len(order):
            a = order[head]
            head += 1
            for b in np.flatnonzero(bonded[a, :Np]):
                if int(b) not in parent_atom:
                    parent_atom[int(b)] = a
                    order.append(int(b))
        if len(order) != Np:
            raise ValueError(f"SubstructureSet: pattern {name!r} is not connected ({len(order)} of its {Np} atoms are "
                             "reached from atom 0)")
        pos = {a: k for k, a in enumerate(order)}
        parent = [pos[parent_atom[a]] for a in order]
        back = [sorted(pos[int(b)] for b in np.flatnonzero(bonded[a, :Np]) if pos[int(b)] < k and pos[int(b)] != parent[k])
                if k else [] for k, a in enumerate(order)]
        return order, parent, back

    def __len__(self):
        return len(self.n_atoms)

    def index(self, which) -> int:
        """A pattern's column from its index or its name."""
        if isinstance(which, str):
            if self.names is None or which not in self.names:
                raise ValueError(f"SubstructureSet: no pattern named {which!r}")
            return self.names.index(which)
        if not isinstance(which, (int, np.integer)) or isinstance(which, bool) or not 0 <= which < len(self):
            raise ValueError(f"SubstructureSet: pattern {which!r} is not an index in [0, {len(self)}) or a name")
        return int(which)

    @classmethod
    def from_molecules(cls, nodes, edges, n_nodes, rules, relax_bonds: bool = False, any_charge: bool = False, *,
                       names=None, device="rules"):
        """One pattern per molecule (int8 or fp32 ``nodes`` [P, N, Fn] / ``edges`` [P, N, N, Fe] as they come from
        anywhere in the library, on the device or the host; ``n_nodes`` [P] or ``None``: the leading rows with a set
        entry): every atom asks for its type and its charge (``any_charge``: for its type only), every bond for its
        type (``relax_bonds``: for any bond, the answer to Kekule phases; both options take one bool or one per
        pattern).  Read back once, here.  A molecule of more
        than 32 atoms, without atoms, or with a node row that is not one-hot in its type and charge segments raises
        ``ValueError``."""
        what = "SubstructureSet.from_molecules"
        A, Cn, _ = _rules_groups(what, rules)
        nodes, edges = _sub_array(what, "nodes", nodes, 3), _sub_array(what, "edges", edges, 4)
        P, N, Fn = nodes.shape
        if edges.shape[:3] != (P, N, N) or A + Cn > Fn or P < 1:
            raise ValueError(f"{what}: nodes {nodes.shape} / edges {edges.shape} must be [P, N, Fn] / [P, N, N, Fe] with "
                             f"P >= 1 and hold the rules' segments {rules.groups}")
        present = (nodes != 0).any(axis=2)
        if n_nodes is None:
            n = np.where(present.all(axis=1), N, np.argmin(present, axis=1))
        else:
            n = _sub_array(what, "n_nodes", n_nodes, 1).astype(np.int64)
            if n.shape != (P,):
                raise ValueError(f"{what}: n_nodes has shape {n.shape}, expected ({P},)")
        if n.min() < 1 or n.max() > min(N, L.SUB_MAX_ATOMS):
            raise ValueError(f"{what}: every molecule needs 1 to {min(N, L.SUB_MAX_ATOMS)} atoms, got "
                             f"{int(n.min())} to {int(n.max())}")
        Npm, Fe = int(n.max()), edges.shape[3]
        inside = np.arange(Npm)[None, :] < n[:, None]
        tm, cm = (nodes[:, :Npm, :A] != 0) & inside[..., None], (nodes[:, :Npm, A:A + Cn] != 0) & inside[..., None]
        if ((tm.sum(axis=2) != 1) & inside).any() or ((cm.sum(axis=2) != 1) & inside).any():
            raise ValueError(f"{what}: a node row below n_nodes is not one-hot in its atom type and formal charge segments")
        bm = (edges[:, :Npm, :Npm] != 0) & inside[:, :, None, None] & inside[:, None, :, None]
        try:
            relax, free = (np.broadcast_to(np.asarray(x, bool), (P,)) for x in (relax_bonds, any_charge))
        except ValueError:
            raise ValueError(f"{what}: relax_bonds and any_charge must be a bool or {P} bools, one per pattern") from None
        bm = np.where(relax[:, None, None, None], np.repeat(bm.any(axis=3, keepdims=True), Fe, axis=3), bm)
        # an atom is marked by its type row, so that Np is n even for atoms that ask for nothing else
        return cls(tm, cm & ~free[:, None, None], bm, names=names, device=rules.device if device == "rules" else device)

    @classmethod
    def from_smiles(cls, strings, rules, max_atoms: int = 32, relax_bonds: bool = False, any_charge: bool = False, *,
                    aromatic: str = "error", names=None):
        """One pattern per SMILES string, through ``read_smiles`` (there is no other parser, and NO SMARTS: a string is a
        molecule; ``aromatic="kekulize"`` reads aromatic input into ONE Kekule phase — use ``relax_bonds`` with it).
        Hydrogens, stated or implied, ask for nothing.  A string with a reader error bit raises ``ValueError``."""
        what = "SubstructureSet.from_smiles"
        strings = list(strings)
        if not 1 <= max_atoms <= L.SUB_MAX_ATOMS:
            raise ValueError(f"{what}: max_atoms must be in [1, {L.SUB_MAX_ATOMS}], got {max_atoms!r}")
        nodes, edges, n, status, _ = read_smiles(strings, rules, max_atoms, aromatic=aromatic).host()
        for s, bits in zip(strings, status):
            if bits & L.SMR_READ_ERROR:
                raise ValueError(f"{what}: {s!r} cannot be read: {describe_read_status(int(bits))}")
        return cls.from_molecules(nodes, edges, n, rules, relax_bonds, any_charge,
                                  names=strings if names is None else names)


class SubstructureMatches(_ResultBuffer):
    """What ``substructure`` wrote, on the device, all int32: ``status`` [G], ``match`` / ``n_anchors`` / ``n_limited``
    [G, P], ``anchors`` [G, P, 4] (atom j: bit ``j & 31`` of word ``j >> 5``), ``first`` [G, P, Np_max]; ``host()`` ->
    ``{name: numpy array}``.  ``patterns`` is the set that was searched for (``None`` axis names with ``pattern_index``)."""

    def __init__(self, buf: torch.Tensor, G: int, P: int, Npm: int, patterns=None):
        super().__init__(buf, G, P, Npm)
        self.P, self.patterns = P, patterns

    @staticmethod
    @functools.lru_cache(maxsize=64)
    def layout(G: int, P: int, Npm: int) -> dict:
        return _pack(("status", "int32", (G,)), ("match", "int32", (G, P)), ("n_anchors", "int32", (G, P)),
                     ("n_limited", "int32", (G, P)), ("anchors", "int32", (G, P, 4)), ("first", "int32", (G, P, Npm)))

    @staticmethod
    def _host_result(a):
        return a


def substructure(nodes: torch.Tensor, edges: torch.Tensor, n_nodes: Optional[torch.Tensor], rules: ValenceRules,
                 patterns: SubstructureSet, *, pattern_index: Optional[torch.Tensor] = None,
                 max_steps: int = 4096) -> SubstructureMatches:
    """Which molecule contains which pattern, for all G molecules and P patterns in one launch
    (``gi_mol_substructure``), with no RDKit and no read-back; inputs as ``validity``.

    **THIS IS NOT SMARTS AND NOT RDKit's MATCHER.**  A pattern (``SubstructureSet``) has per atom a set of types, a set
    of charges, an exact degree and a least hydrogen count, and per bond a set of bond types: **no ring or recursive
    predicates, and no aromaticity is perceived** — a Kekule pattern of a fused ring system matches only the molecule's
    stored Kekule phase; ``relax_bonds=True`` is the answer for scaffolds.  A match is a monomorphism, as in
    ``HasSubstructMatch``: the molecule may have more bonds than the pattern.

    The search runs per (molecule, pattern, anchor), the anchor being the image of pattern atom 0, depth first along
    the pattern's plan with candidates in ascending atom index (include/graphinvent_amd.h has the rule,
    tests/substructure_model.py is the specification, matched integer for integer).  An anchor that has taken
    ``max_steps`` steps (1 to 2**20) and needs another is given up: it counts as no match and in ``n_limited``, and the
    molecule gets ``SUB_STEP_LIMIT``.  The 863 DRD2 fixture molecules against 18 usual groups and scaffolds never pass
    112 steps.

    Result (``SubstructureMatches``, views of one device buffer, ``.host()`` is one copy): ``match`` [G, P] 0 / 1;
    ``n_anchors`` [G, P] the atoms that are the image of pattern atom 0 in some match (the functional-group count when
    atom 0 is the group's centre); ``anchors`` [G, P, 4] the same as a 128-bit mask; ``first`` [G, P, Np_max] the images
    of the pattern's atoms, in the pattern's own atom order, found from the lowest matching anchor (-1 where none and
    past Np); ``n_limited`` [G, P]; ``status`` [G] (``SUBSTRUCTURE_STATUS_MESSAGES``): a malformed, empty or self-loop
    molecule matches nothing.  With ``pattern_index`` (int32 [G], on the device) molecule g is searched for pattern
    ``pattern_index[g]`` only and the P axis has length 1 (is the seed still in its product); an index outside [0, P)
    gives no match and ``SUB_PATTERN_INDEX``.  G = 0 is answered without a launch."""
    what = "substructure"
    _rules_groups(what, rules)
    if not isinstance(patterns, SubstructureSet):
        raise TypeError(f"{what}: patterns must be a SubstructureSet, got {type(patterns).__name__}")
    if (not isinstance(max_steps, (int, np.integer)) or isinstance(max_steps, bool)
            or not 1 <= max_steps <= L.SUB_MAX_STEPS):
        raise ValueError(f"{what}: max_steps must be an integer in [1, {L.SUB_MAX_STEPS}], got {max_steps!r}")
    G, N, Fn, Fe, dtype, n_nodes, nn_bytes, _ = _check_inputs(what, nodes, edges, n_nodes, None, False)
    dev = nodes.device
    A, Cn, H, order2 = _check_rules(what, rules, Fn, Fe, dev)
    if patterns.dims != (A, Cn, Fe):
        raise ValueError(f"{what}: the patterns were built for (types, charges, bond types) = {patterns.dims}, the "
                         f"molecules and rules have {(A, Cn, Fe)}")
    if patterns.table_dev is None:
        raise RuntimeError(f"{what}: the patterns were built with device=None and hold no device table (no CPU fallback)")
    if patterns.table_dev.device != dev:
        raise ValueError(f"{what}: the molecules are on {dev}, the patterns on {patterns.table_dev.device}")
    if pattern_index is not None:
        if not isinstance(pattern_index, torch.Tensor) or not pattern_index.is_cuda or pattern_index.device != dev:
            raise RuntimeError(f"{what}: pattern_index must be a CUDA tensor on {dev} (no CPU fallback)")
        if (tuple(pattern_index.shape) != (G,) or pattern_index.dtype != torch.int32
                or not pattern_index.is_contiguous()):
            raise ValueError(f"{what}: pattern_index must be a contiguous int32 tensor of shape ({G},), got "
                             f"{pattern_index.dtype} {tuple(pattern_index.shape)}")
    P = 1 if pattern_index is not None else len(patterns)
    res = SubstructureMatches.empty(dev, G, P, patterns.Np_max, patterns=None if pattern_index is not None else patterns)
    if G > 0:
        out = res._ptrs()
        with torch.cuda.device(dev):
            L.check(L.load().gi_mol_substructure(
                G, N, Fn, Fe, nodes.data_ptr(), edges.data_ptr(), dtype,
                None if n_nodes is None else n_nodes.data_ptr(), nn_bytes, A, Cn, H, rules.allowed_mask.data_ptr(),
                order2.data_ptr(), patterns.table.ctypes.data, patterns.table_dev.data_ptr(), patterns.table.size,
                None if pattern_index is None else pattern_index.data_ptr(), int(max_steps), out["match"],
                out["n_anchors"], out["anchors"], out["first"], out["n_limited"], out["status"],
                torch.cuda.current_stream(dev).cuda_stream), "gi_mol_substructure")
    return res


def _column_runs(cols):
    """Sorted distinct columns as (start, stop) runs: a slice each, no index tensor to copy to the device."""
    runs = []
    for c in sorted(set(cols)):
        if runs and runs[-1][1] == c:
            runs[-1][1] = c + 1
        else:
            runs.append([c, c + 1])
    return runs


def substructure_score(result: SubstructureMatches, *, require=(), forbid=()) -> torch.Tensor:
    """A contribution for ``compute_score``: fp32 [G], 1 where every ``require`` pattern matches and no ``forbid``
    pattern does, else 0 (pattern indices, or names of a named set).  Plain torch on ``result.match``'s device, no
    read-back.  A molecule that matches nothing (malformed, empty) passes a forbid-only list: mask it with ``validity``,
    as ``compute_score`` does."""
    what = "substructure_score"
    if not isinstance(result, SubstructureMatches):
        raise TypeError(f"{what}: result must be substructure's result, got {type(result).__name__}")
    if result.patterns is None:
        raise ValueError(f"{what}: a result made with pattern_index has one column; use result.match[:, 0]")
    req, forb = ([result.patterns.index(w) for w in which] for which in (require, forbid))
    m = result.match
    ok = torch.ones(result.G, dtype=torch.bool, device=m.device)
    for a, b in _column_runs(req):
        ok = ok & (m[:, a:b] != 0).all(dim=1)
    for a, b in _column_runs(forb):
        ok = ok & (m[:, a:b] == 0).all(dim=1)
    return ok.to(torch.float32)


# ---- the resonance normal form: one identity per compound --------------------------------------------------------------
#: status bits of ``resonance`` / ``kekulize`` / ``canonical_compound`` beyond the malformed bits
RESONANCE_STATUS_MESSAGES = {
    **{bit: VALIDITY_STATUS_MESSAGES[bit] for bit in (L.MOL_ONEHOT, L.MOL_BOND_PAST_N, L.MOL_VALUE, L.MOL_MULTI_BOND,
                                                      L.MOL_ASYMMETRIC, L.MOL_NODE_PAST_N)},
    L.RES_EMPTY: "the molecule has no atoms: nothing is delocalised",
    L.RES_SELF_LOOP: "an atom is bonded to itself: nothing is delocalised, the edges are copied",
    L.RES_AROMATIC: "a stored bond of order 1.5 is present: left as it is, its atoms take no part (informational)",
    L.RES_BOND_ORDER: "kekulize: there are delocalised bonds and the rules lack a bond type of order 1 or of order 2",
    L.RES_NO_KEKULE: "kekulize: the delocalised bonds have no perfect matching (no Kekule structure)",
}
#: the bits after which ``kekulize`` writes all-zero edges
NO_KEKULE_BITS = MALFORMED_BITS | L.RES_EMPTY | L.RES_SELF_LOOP | L.RES_BOND_ORDER | L.RES_NO_KEKULE


def describe_resonance_status(bits: int) -> str:
    return "; ".join(msg for bit, msg in RESONANCE_STATUS_MESSAGES.items() if bits & bit) or "well-formed"


class ResonanceForms(_ResultBuffer):
    """What ``resonance`` wrote, on the device: ``status`` / ``n_delocalized`` (bonds) / ``n_atoms`` / ``n_systems``
    (connected components of the delocalised bonds) [G] int32 and ``delocalized`` [G, N, 4] int32 (128-bit rows: bit
    ``j & 31`` of word ``j >> 5`` of row i = bond i-j is delocalised, the layout of ``substructure``'s ``anchors``) as
    views of one buffer (``host()`` -> ``{name: numpy array}`` of the five); and ``.edges`` [G, N, N, Fe + 1] int8, the
    normal form, when asked for (``None`` otherwise; not part of ``host()``)."""

    def __init__(self, buf: torch.Tensor, G: int, N: int, edges=None):
        super().__init__(buf, G, N)
        self.N, self.edges = N, edges

    @staticmethod
    @functools.lru_cache(maxsize=64)
    def layout(G: int, N: int) -> dict:
        return _pack(("status", "int32", (G,)), ("n_delocalized", "int32", (G,)), ("n_atoms", "int32", (G,)),
                     ("n_systems", "int32", (G,)), ("delocalized", "int32", (G, N, 4)))

    @staticmethod
    def _host_result(a):
        return a


def _check_normal_form_width(what: str, edges, extra: int):
    """``Fe + 1 > GI_MAX_GROUPS`` is refused before anything else looks at the tensors (and before any launch)."""
    if isinstance(edges, torch.Tensor) and edges.dim() == 4 and edges.shape[3] + extra > L.GI_MAX_GROUPS:
        raise ValueError(f"{what}: the normal form has one channel more than the Fe = {edges.shape[3] + extra - 1} bond "
                         f"types, which exceeds the limit of {L.GI_MAX_GROUPS} channels")


def resonance(nodes: torch.Tensor, edges: torch.Tensor, n_nodes: Optional[torch.Tensor], rules: ValenceRules, *,
              want_edges: bool = True) -> ResonanceForms:
    """Which bonds change order between the Kekule structures of each molecule, and the molecules in RESONANCE NORMAL
    FORM, in one launch (``gi_mol_resonance``) with no read-back; inputs as ``validity``.

    **THIS IS NOT AROMATICITY PERCEPTION, and not RDKit's.**  No Hueckel count, no chemistry table, no moving charges,
    no tautomers: cyclobutadiene, cyclooctatetraene and pentalene are delocalised; pyrrole, furan, quinone and the
    five-ring of indole are not, because they have ONE Kekule structure and identity needs nothing there.  The rule
    (include/graphinvent_amd.h at ``gi_mol_resonance``; tests/resonance_model.py is the specification): among the atoms
    with exactly one double bond, no triple or 1.5 bond, and a double-bond partner of the same kind, a single or double
    bond is DELOCALISED iff it lies on a cycle of alternating single and double bonds — iff the molecule has a Kekule
    structure in which that bond has the other order.  Consequences: all Kekule structures of one compound have the
    same normal form, byte for byte, and equal normal forms mean Kekule structures of one compound; no acyclic bond is
    delocalised; every atom's bond-order sum is unchanged.  A stored 1.5 bond is left alone (``RES_AROMATIC``).

    ``.edges`` [G, N, N, Fe + 1] int8 is the normal form: a delocalised bond has channel ``Fe`` set and no other, every
    other bond is as stored (``Fe + 1 > GI_MAX_GROUPS`` raises ``ValueError``; ``want_edges=False`` writes none).
    IDENTITY PER COMPOUND is composition, the entry points of ``canonical`` are unchanged::

        r = resonance(nodes, edges, n_nodes, rules)
        uniq, rep, n_classes = unique(nodes, r.edges, n_nodes, mask=valid)      # likewise fraction_unique, canonical
        new = seen.add(nodes, r.edges, n_nodes, mask=valid)                     # a SeenSet of normal forms

    (``r.edges`` is int8 whatever the input's dtype; fp32 node states go with it as ``nodes.to(torch.int8)``.)

    ``status`` (``RESONANCE_STATUS_MESSAGES``): the malformed bits, ``RES_EMPTY``, ``RES_SELF_LOOP`` (any of them:
    nothing is delocalised and the edges are copied, so ``canonical`` says about the normal form what it says about
    the input) and ``RES_AROMATIC``.  ``delocalized`` is the mask a phase-independent substructure search would take;
    feeding it to ``substructure`` is not done here."""
    what = "resonance"
    _rules_groups(what, rules)
    if want_edges:
        _check_normal_form_width(what, edges, 1)
    G, N, Fn, Fe, dtype, n_nodes, nn_bytes, _ = _check_inputs(what, nodes, edges, n_nodes, None, False)
    dev = nodes.device
    A, Cn, H, order2 = _check_rules(what, rules, Fn, Fe, dev)
    out_e = torch.empty((G, N, N, Fe + 1), dtype=torch.int8, device=dev) if want_edges else None
    res = ResonanceForms.empty(dev, G, N, edges=out_e)
    if G > 0:
        out = res._ptrs()
        with torch.cuda.device(dev):
            L.check(L.load().gi_mol_resonance(
                G, N, Fn, Fe, nodes.data_ptr(), edges.data_ptr(), dtype,
                None if n_nodes is None else n_nodes.data_ptr(), nn_bytes, A, Cn, H, order2.data_ptr(), out["status"],
                out["n_delocalized"], out["n_atoms"], out["n_systems"], out["delocalized"],
                None if out_e is None else out_e.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
                "gi_mol_resonance")
    return res


def kekulize(nodes: torch.Tensor, edges: torch.Tensor, n_nodes: Optional[torch.Tensor], rules: ValenceRules):
    """The inverse of ``resonance``: molecules in normal form (``edges`` [G, N, N, Fe + 1], fp32 or int8, the rules
    holding ``Fe`` bond orders) -> ``(edges [G, N, N, Fe] int8, status [G] int32)``, one launch (``gi_mol_kekulize``),
    no read-back.  Every atom on a channel-``Fe`` bond gets exactly one double bond among those bonds: a perfect
    matching found as the SMILES reader's kekuliser finds it (greedy in ascending index, then augmenting paths with
    blossom contraction, neighbours ascending), the other channel-``Fe`` bonds become single.  THE CHOICE IS A FUNCTION
    OF THE INDEXED GRAPH, not a chemical preference: on canonical molecules it is a canonical Kekule structure
    (``canonical_compound``).  ``status``: ``RES_NO_KEKULE`` (no perfect matching), ``RES_BOND_ORDER`` (no single or
    no double type in the rules), the malformed bits, ``RES_EMPTY``, ``RES_SELF_LOOP`` — after any of them
    (``NO_KEKULE_BITS``) the molecule's edges are all zero — and ``RES_AROMATIC``."""
    what = "kekulize"
    _rules_groups(what, rules)
    _check_normal_form_width(what, edges, 0)
    G, N, Fn, Fi, dtype, n_nodes, nn_bytes, _ = _check_inputs(what, nodes, edges, n_nodes, None, False)
    if Fi < 2:
        raise ValueError(f"{what}: edges must hold Fe + 1 >= 2 channels (the bond types and the delocalised channel)")
    dev = nodes.device
    A, Cn, H, order2 = _check_rules(what, rules, Fn, Fi - 1, dev)
    out_e = torch.empty((G, N, N, Fi - 1), dtype=torch.int8, device=dev)
    status = torch.empty(G, dtype=torch.int32, device=dev)
    if G > 0:
        with torch.cuda.device(dev):
            L.check(L.load().gi_mol_kekulize(
                G, N, Fn, Fi - 1, nodes.data_ptr(), edges.data_ptr(), dtype,
                None if n_nodes is None else n_nodes.data_ptr(), nn_bytes, A, Cn, H, order2.data_ptr(),
                status.data_ptr(), out_e.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "gi_mol_kekulize")
    return out_e, status


def canonical_compound(nodes: torch.Tensor, edges: torch.Tensor, n_nodes: Optional[torch.Tensor], rules: ValenceRules):
    """One representative per COMPOUND: ``resonance`` -> ``canonical(..., want_molecules=True)`` on the normal form ->
    ``kekulize`` of the canonical molecules; three launches, no read-back.  -> ``(nodes [G, N, Fn] int8, edges
    [G, N, N, Fe] int8, key [G, 2] int64, status [G] int32)``: the canonical nodes, the canonical Kekule structure (a
    molecule every other entry point takes: ``smiles`` of it writes ONE string per compound, whatever the node order
    and the stored phase of the input), ``canonical``'s key of the normal form, and ``resonance``'s status with
    ``canonical``'s bits and ``kekulize``'s ``RES_NO_KEKULE`` / ``RES_BOND_ORDER`` added.  A molecule with a malformed
    bit has zero nodes and edges, as in ``canonical``; ``canonical``'s completeness caveat applies unchanged."""
    r = resonance(nodes, edges, n_nodes, rules)
    if nodes.dtype != torch.int8:                            # the normal form is int8: 0, 1, and 2 for any other entry
        nodes = nodes.ne(0).to(torch.int8) + (nodes.ne(0) & nodes.ne(1)).to(torch.int8)
    can = canonical(nodes, r.edges, n_nodes, want_molecules=True)
    k_edges, k_status = kekulize(can.nodes, can.edges, n_nodes, rules)
    status = r.status | can.status | (k_status & (L.RES_NO_KEKULE | L.RES_BOND_ORDER))
    return can.nodes, k_edges, can.key, status
