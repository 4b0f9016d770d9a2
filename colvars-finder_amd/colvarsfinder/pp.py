"""Preprocessing layer ``r(x)``: Kabsch alignment to a reference structure + feature map.

The reference takes this layer from the third-party package molann
(``examples/dipeptide/main.ipynb:31-32,333-348``) and treats it as an opaque
``pp_layer: torch.nn.Module`` (``core.py:65,122,403,414,635``).  This module provides the same
constructor surface (``Feature``, ``FeatureLayer``, ``AlignmentLayer``, ``PreprocessingANN``;
atom groups are duck-typed: ``.ix`` and ``.positions``) on top of :class:`AlignFeatureLayer`,
whose ``forward`` is the hand-written gfx950 kernel K1 behind ``cvf_align_feature_fwd``.

Conventions: unweighted centroid of the align atoms,
``x_aligned = (x - c) @ R`` with ``R = U diag(1,1,sign det(U V^T)) V^T`` from the SVD of
``(x_align - c)^T @ ref_c``; features are concatenated in list order: ``position`` -> 3 n
coordinates (atom-major), ``bond`` -> distance, ``angle`` -> cos (or value), ``dihedral`` ->
(cos, sin) (or value).
"""

import copy

import numpy as np
import torch

from . import _hip

_TYPE_ID = {"angle": _hip.FEAT_ANGLE, "bond": _hip.FEAT_BOND, "dihedral": _hip.FEAT_DIHEDRAL,
            "position": _hip.FEAT_POSITION}
_TYPE_NATOMS = {"angle": 3, "bond": 2, "dihedral": 4}


def _ix(atom_group):
    return np.asarray(atom_group.ix if hasattr(atom_group, "ix") else atom_group, dtype=np.int64)


def _batch_records(recs, width=64):
    """Slot records ``[type, s0, s1, s2, s3, out]``, sorted by type, in batches of ``width`` of ONE type (the streaming
    alignment kernel hands a batch to the lanes of a wave: one code path per wave); short batches are padded with
    ``type = -1`` entries (CVF_PP_SLOT_BATCHED)."""
    out, i = [], 0
    while i < len(recs):
        j = i
        while j < len(recs) and recs[j][0] == recs[i][0] and j - i < width:
            j += 1
        out += [list(r) for r in recs[i:j]] + [[-1, 0, 0, 0, 0, 0]] * (width - (j - i))
        i = j
    return out


class Feature:
    """``Feature(name, feature_type, atom_group)`` as in molann (main.ipynb:335)."""

    def __init__(self, name, feature_type, atom_group):
        if feature_type not in _TYPE_ID:
            raise ValueError(f"unknown feature type '{feature_type}' (expected one of {sorted(_TYPE_ID)})")
        idx = _ix(atom_group)
        if feature_type != "position" and len(idx) != _TYPE_NATOMS[feature_type]:
            raise ValueError(f"feature '{name}' of type {feature_type} needs {_TYPE_NATOMS[feature_type]} atoms, got {len(idx)}")
        self.name, self.type_name, self.type_id, self.atom_indices = name, feature_type, _TYPE_ID[feature_type], idx

    def get_name(self):
        return self.name

    def get_type(self):
        return self.type_name

    def get_atom_indices(self):
        return self.atom_indices


class AlignFeatureLayer(torch.nn.Module):
    """Alignment + features on local (0-based, into the input atoms) indices.

    Args:
        n_atoms: number of input atoms N; ``forward`` takes ``[B, N, 3]``.
        align_idx: local indices of the atoms used for the alignment, or ``None``: no alignment - the features are those of
            the raw coordinates (molann's ``PreprocessingANN(None, feature_layer)``; ``CVF_PP_FEATURES``, csrc/k1_features.hip),
            a ``position`` feature returns ``x[:, atoms]`` unchanged.  ``ref_pos`` and ``align_weights`` must then be ``None``.
        ref_pos: ``[n_align, 3]`` reference positions of those atoms (stored centred).
        features: list of ``(type_name, local_atom_indices)``.
        use_angle_value: emit angles in radians instead of cos / (cos, sin).
        align_weights: optional ``[n_align]`` non-negative per-atom weights w_b of the alignment (masses, say): the
            frame's weighted centroid goes to the reference's and the rotation minimises
            ``sum_b w_b |(x_b - c) R - ref_b|^2``.  ``None`` = the uniform weights of molann's layer.  Weighted layers
            of at most 64 atoms run on the general lane-per-frame kernels; larger ones need ``weights_any_size``.
        weights_any_size: opt-in, like ``general_nets=True`` of the tasks: a weighted layer of MORE than 64 atoms is built for
            the streaming kernels of large molecules (csrc/k1_large.hip and the large-frame derivative kernels), which take
            the weights at any size.  The table flags (contiguous align set, batched slot records) are kept - they describe
            the tables, not the weights.  With at most 64 atoms the option changes nothing; without it such a layer is
            refused as before.
        second_order: ``None`` (default), ``"cotangent"`` or ``"complete"``; also a settable attribute
            (``layer.second_order = "complete"``, the way to set it on a :class:`PreprocessingANN`).  ``None``: the layer is
            differentiable to first order and its backward raises under ``create_graph=True``.  ``"cotangent"``: the backward
            ``gx = J(x)^T g`` is itself recorded, as a function of its cotangent ``g`` - enough for every loss of the coordinate
            gradient ``L(grad_x f_theta(r(x)))`` that is differentiated in the net's parameters, because the layer has none and
            ``g -> J(x)^T g`` is linear (its derivative is the HIP Jacobian-vector product ``cvf_align_feature_jvp``).  The
            other half of the second derivative, the curvature term ``d/dx (v^T J(x)^T g)``, is left out: a backward that
            reaches ``x`` through this path fills ``x.grad`` with NaN instead of a number that would be silently wrong.
            ``"complete"``: the curvature term is there as well, from the HIP Hessian-vector product
            ``cvf_align_feature_hvp`` - a double backward gives exact gradients in the coordinates too (a trainable module in
            front of the layer under a gradient loss, ``grad_x |grad_x xi|^2``, a Hessian of ``xi`` row by row), and
            ``torch.autograd.forward_ad`` over the backward works.  The gradients that reach the layer through the cotangent
            are those of ``"cotangent"``, bit for bit.  Third derivatives are not built: differentiating the curvature term
            once more raises.
    """

    def __init__(self, n_atoms, align_idx, ref_pos, features, use_angle_value=False, align_weights=None, weights_any_size=False,
                 second_order=None):
        super().__init__()
        self.second_order = second_order
        self.aligned = align_idx is not None
        if not self.aligned:
            assert ref_pos is None, "ref_pos without align_idx: a layer without alignment has no reference structure"
            assert align_weights is None, "align_weights without align_idx: a layer without alignment has no alignment weights"
            align_idx, ref_pos = np.zeros(0, dtype=np.int64), np.zeros((0, 3))
        align_idx = np.asarray(align_idx, dtype=np.int64)
        ref = np.asarray(ref_pos, dtype=np.float64)
        assert ref.shape == (len(align_idx), 3), f"ref_pos must be [{len(align_idx)},3], got {ref.shape}"
        if self.aligned:
            assert len(align_idx) >= 3, "at least 3 atoms are needed for the alignment"
            assert align_idx.min() >= 0 and align_idx.max() < n_atoms, "align index out of range"
        rec, out = [], 0
        for tname, atoms in features:
            atoms = [int(a) for a in atoms]
            assert all(0 <= a < n_atoms for a in atoms), f"feature atom index out of range: {atoms}"
            if tname == "position":
                for a in atoms:
                    rec.append([_hip.FEAT_POSITION, a, 0, 0, 0, out])
                    out += 3
            else:
                assert len(atoms) == _TYPE_NATOMS[tname]
                rec.append([_TYPE_ID[tname]] + atoms + [0] * (4 - len(atoms)) + [out])
                out += 2 if (tname == "dihedral" and not use_angle_value) else 1
        self.n_atoms, self.d_r, self.use_angle_value = int(n_atoms), out, bool(use_angle_value)
        self.features = [(t, tuple(int(a) for a in atoms)) for t, atoms in features]
        # structure hints for the kernels (include/cvf.h): affine tables allow the fast kernels
        flags = 0
        if self.aligned and np.array_equal(align_idx, np.arange(len(align_idx))):
            flags |= _hip.PP_ALIGN_CONTIG
        if self.aligned and all(r[0] == _hip.FEAT_POSITION and r[1] == i and r[5] == 3 * i for i, r in enumerate(rec)):
            flags |= _hip.PP_PURE_POSITION
        # per-atom weights: the kernels take them with mean 1, and the reference positions centred by their WEIGHTED
        # centroid and pre-multiplied by them (include/cvf.h, cvf_pp_desc.align_w) - the covariance
        # sum_b w_b (x_b - c) (x) ref_b is then the same loop as the unweighted one
        w_hat = None
        weighted_large = align_weights is not None and bool(weights_any_size) and 3 * n_atoms > 192
        if align_weights is not None:
            w = np.asarray(align_weights, dtype=np.float64).reshape(-1)
            assert w.shape == (len(align_idx),), f"align_weights must be [{len(align_idx)}], got {w.shape}"
            assert np.all(np.isfinite(w)) and np.all(w >= 0) and np.count_nonzero(w) >= 3, \
                "align_weights must be finite, non-negative, with at least 3 non-zero entries"
            assert weighted_large or 3 * n_atoms <= 192, "weighted alignment is built for frames of at most 64 atoms"
            w_hat = w * (len(w) / w.sum())
            if weighted_large:   # the streaming kernels: the table flags stay, PURE_POSITION means nothing there
                flags &= _hip.PP_ALIGN_CONTIG
            else:
                flags = 0   # the fast layouts assume uniform weights
        self._flags = flags
        # per-atom tables for the streaming kernel of large molecules (include/cvf.h): which ref row an atom aligns
        # to, and the compact "slot" of every atom some feature reads
        atom_align = np.full(n_atoms, -1, dtype=np.int32)
        atom_align[align_idx] = np.arange(len(align_idx), dtype=np.int32)
        used = sorted({int(a) for r in rec for a in (r[1:2] if r[0] == _hip.FEAT_POSITION else
                                                      r[1:1 + _TYPE_NATOMS[{v: k_ for k_, v in _TYPE_ID.items()}[r[0]]]])})
        atom_slot = np.full(n_atoms, -1, dtype=np.int32)
        atom_slot[used] = np.arange(len(used), dtype=np.int32)
        rec_slot = []
        for r in rec:
            na = 1 if r[0] == _hip.FEAT_POSITION else _TYPE_NATOMS[{v: k_ for k_, v in _TYPE_ID.items()}[r[0]]]
            rec_slot.append([r[0]] + [int(atom_slot[a]) for a in r[1:1 + na]] + [0] * (4 - na) + [r[5]])
        # the streaming kernel hands one record to each lane, 64 at a time: records of one type side by side keep a
        # wave's lanes on one code path (CVF_PP_SLOT_BATCHED; the output offset travels with the record, so the order is
        # free; type -1 entries are padding)
        by_type = sorted(rec_slot, key=lambda r: r[0])
        rec_slot = _batch_records(by_type)
        if (w_hat is None or weighted_large) and self.aligned:
            self._flags |= _hip.PP_SLOT_BATCHED
        self._n_rec_slot = len(rec_slot)
        self._n_slot = len(used)
        # the derivative kernel of large molecules (csrc/metric_large.hip) scatters J^T g through a table of rows: one row per
        # (record, atom position) pair, the rows of one slot contiguous (include/cvf.h: mrec, slot_row)
        natoms = {_hip.FEAT_POSITION: 1, _hip.FEAT_BOND: 2, _hip.FEAT_ANGLE: 3, _hip.FEAT_DIHEDRAL: 4}
        pairs = sorted((r[1 + j], i, j) for i, r in enumerate(by_type) for j in range(natoms[r[0]]))   # (slot, record, position)
        row_of = {(i, j): n for n, (_, i, j) in enumerate(pairs)}
        slot_row = np.zeros(len(used) + 1, dtype=np.int32)
        for t, _, _ in pairs:
            slot_row[t + 1] += 1
        slot_row = np.cumsum(slot_row).astype(np.int32)
        mrec = []
        for i, r in enumerate(by_type):
            na = natoms[r[0]]
            rows = [row_of[(i, j)] for j in range(na)] + [0] * (4 - na)
            ur = [int(slot_row[r[1 + j]]) for j in range(na)] + [0] * (4 - na)
            sl = list(r[1:5])
            off = [rows[j] - ur[j] if j < na else 0 for j in range(4)]     # position of this record among its atom's rows
            self._row_off_max = max(getattr(self, "_row_off_max", 0), max(off))
            mrec.append([(r[0] + 1) | (r[5] << 3), sl[0] | (sl[1] << 16), sl[2] | (sl[3] << 16), ur[0] | (ur[1] << 16),
                         ur[2] | (ur[3] << 16), off[0] | (off[1] << 8) | (off[2] << 16) | (off[3] << 24), 0, 0])
        self._n_ref = len(pairs)
        self.register_buffer("mrec", torch.tensor(np.asarray(mrec, dtype=np.int64).astype(np.uint32).view(np.int32)
                                                  if mrec else np.zeros((0, 8), np.int32)).reshape(-1, 8))
        self.register_buffer("slot_row", torch.tensor(slot_row, dtype=torch.int32))
        self.register_buffer("atom_align", torch.tensor(atom_align))
        self.register_buffer("atom_slot", torch.tensor(atom_slot))
        self.register_buffer("rec_slot", torch.tensor(rec_slot, dtype=torch.int32).reshape(-1, 6))
        self.register_buffer("slot_atom", torch.tensor(used, dtype=torch.int32))
        self.register_buffer("align_idx", torch.tensor(align_idx, dtype=torch.int32))
        if not self.aligned:
            ref_c, self.align_w = ref, None
        elif w_hat is None:
            ref_c = ref - ref.mean(axis=0, keepdims=True)
            self.align_w = None
        else:
            ref_c = w_hat[:, None] * (ref - (w_hat[:, None] * ref).mean(axis=0, keepdims=True))
            self.register_buffer("align_w", torch.tensor(w_hat, dtype=torch.float32))
        self.register_buffer("ref_c", torch.tensor(ref_c, dtype=torch.float32))
        self.register_buffer("rec", torch.tensor(rec, dtype=torch.int32).reshape(-1, 6))

    @property
    def second_order(self):
        return self.__dict__.get("_second_order")   # (a layer pickled before the option existed: None)

    @second_order.setter
    def second_order(self, value):
        if value not in _SECOND_ORDER:
            raise ValueError(f"second_order must be one of {_SECOND_ORDER}, got {value!r}")
        self._second_order = value

    def derivative_table_limits(self):
        """None, or why the large-molecule derivative kernel (csrc/metric_large.hip: metric_rows_kernel) cannot take this feature
        list: its tables pack a record's slots and rows into 16-bit fields, a record's position among its atom's rows into 8 bits
        and a slot's row count into 12 bits.  EigenFunctionTask's generator mode asks at construction."""
        if not self.aligned:   # features of the raw coordinates (csrc/k1_features.hip): the limits of include/cvf.h
            for what, have, limit in (("distinct feature atoms (n_slot)", self._n_slot, _hip.FEATURES_MAX_SLOT),
                                      ("contribution rows (n_ref: atoms summed over the features)", self._n_ref, _hip.FEATURES_MAX_REF)):
                if have > limit:
                    return f"{have} {what}; the kernels of a layer without alignment take at most {limit}"
            if getattr(self, "_row_off_max", 0) >= 256:
                return f"{self._row_off_max + 1} features that share one atom; the derivative kernel's tables hold fewer than 256"
            return None
        rows_per_slot = int(np.diff(np.concatenate([[0], self.slot_row.cpu().numpy()])).max()) if self.slot_row.numel() else 0
        for what, have, limit in (("contribution rows (atoms summed over the features)", self._n_ref, 65536),
                                  ("distinct feature atoms", self._n_slot, 65536),
                                  ("features that share one atom", getattr(self, "_row_off_max", 0) + 1, 256),
                                  ("contribution rows of one atom", rows_per_slot, 4096)):
            if have >= limit:
                return f"{have} {what}; the derivative kernel's tables hold fewer than {limit}"
        return None

    def pp_desc(self):
        assert self.rec.is_cuda, "preprocessing layer is not on the GPU (call .to(device))"
        d = _hip.PPDesc()
        d.mode, d.n_coord, d.n_align, d.n_rec = _hip.PP_ALIGN if self.aligned else _hip.PP_FEATURES, 3 * self.n_atoms, self.align_idx.numel(), self.rec.shape[0]
        d.d_r, d.use_angle_value = self.d_r, int(self.use_angle_value)
        d.has_position = int(bool((self.rec[:, 0] == _hip.FEAT_POSITION).any().item()))
        d.flags = self._flags
        d.rec, d.atom_slot, d.rec_slot = self.rec.data_ptr(), self.atom_slot.data_ptr(), self.rec_slot.data_ptr()
        if self.aligned:
            d.align_idx, d.ref_c, d.atom_align = self.align_idx.data_ptr(), self.ref_c.data_ptr(), self.atom_align.data_ptr()
        d.slot_atom, d.n_slot, d.n_rec_slot = self.slot_atom.data_ptr(), self._n_slot, self._n_rec_slot
        d.align_w = self.align_w.data_ptr() if self.align_w is not None else None
        if self._n_ref < 65536 and self._n_slot < 65536 and getattr(self, "_row_off_max", 0) < 256:   # (else: cvf_metric_apply names what is missing)
            d.mrec, d.slot_row, d.n_mrec, d.n_ref = self.mrec.data_ptr(), self.slot_row.data_ptr(), self.mrec.shape[0], self._n_ref
        return d

    def forward(self, x):
        """``[B, N, 3]`` -> ``[B, d_r]``.  The reference calls this layer (through ``colvar_model()``) on CPU tensors
        made from the trajectory (2d.ipynb:437-446, main.ipynb:561-562): the frames are moved to the layer's GPU, run
        through kernel K1 and the features come back on the input's device in the input's floating-point type.

        Differentiable in ``x`` to first order, like molann's layer: when ``x`` requires grad (and grad mode is on) the call
        records a graph whose backward runs the HIP vector-Jacobian product ``cvf_align_feature_vjp`` and returns ``dL/dx`` in
        ``x``'s type and on ``x``'s device.  Forward mode works the same way: under ``torch.autograd.forward_ad`` a dual input
        gives a dual output whose tangent ``J(x) v`` is the HIP Jacobian-vector product ``cvf_align_feature_jvp``, in the
        input's type and on its device.

        Second derivatives are opt-in.  By default (``second_order=None``) the backward raises under ``create_graph=True``;
        ``colvar_model()`` with a grad-requiring input and ``export.ScriptableAlignFeature`` have them in torch operators.
        With ``second_order="cotangent"`` the backward is recorded as a function of its cotangent, which is all that a loss of
        ``grad_x f_theta(layer(x))`` needs for its gradient in ``theta``; ``x.grad`` after such a backward is NaN (the curvature
        term of the layer is left out, and NaN rather than a wrong number says so).  With ``second_order="complete"`` the
        curvature term comes from the HIP Hessian-vector product ``cvf_align_feature_hvp`` and ``x.grad`` is exact; third
        derivatives raise.  The training tasks use the analytic derivative kernels and call this layer without a graph."""
        x = torch.as_tensor(x)
        dev = _hip.require_gpu(self.rec.device)   # raises when the layer was never moved to a GPU: there is no CPU path
        assert x.dim() == 3 and x.shape[1] == self.n_atoms and x.shape[2] == 3, \
            f"expected [B,{self.n_atoms},3], got {tuple(x.shape)}"
        src_dev, src_dt = x.device, (x.dtype if x.dtype.is_floating_point else torch.float32)
        if (x.requires_grad and torch.is_grad_enabled()) or _has_tangent(x):
            # the conversions stay on the graph: a CPU fp64 input receives a CPU fp64 gradient
            xd = x.to(device=dev, dtype=torch.float32).contiguous()
            out = _AlignFeatureFn.apply(xd, self)
            return out.to(device=src_dev, dtype=src_dt)
        x = x.detach().to(device=dev, dtype=torch.float32).contiguous()
        B = x.shape[0]
        out = torch.empty(B, self.d_r, device=dev, dtype=torch.float32)
        if B > 0:
            with torch.cuda.device(dev):
                desc = self.pp_desc()
                scratch = _hip.align_scratch(desc, B, dev)
                _hip.check(_hip.lib().cvf_align_feature_fwd(desc, _hip.ptr(x), B, None, _hip.ptr(out), None, _hip.ptr(scratch),
                                                            _hip.stream()), "cvf_align_feature_fwd")
        return out.to(device=src_dev, dtype=src_dt)


_NO_DOUBLE_BACKWARD = ("AlignFeatureLayer: second derivatives through the HIP alignment + feature layer are not built (its "
                       "backward ran with create_graph=True); differentiate twice through colvar_model() called with a "
                       "grad-requiring input, or through export.ScriptableAlignFeature(layer), which are written with torch "
                       "operators. A loss of the coordinate gradient that is differentiated in the net's parameters only "
                       "runs on the HIP layer with layer.second_order = 'cotangent' (x.grad is then NaN); "
                       "layer.second_order = 'complete' adds the curvature term (cvf_align_feature_hvp), so that the "
                       "coordinates receive their exact second-order gradient as well")
_NO_THIRD_ORDER = ("AlignFeatureLayer: third derivatives through the HIP alignment + feature layer are not built (the "
                   "Hessian-vector product cvf_align_feature_hvp of second_order='complete' was differentiated once more); "
                   "export.ScriptableAlignFeature(layer), written with torch operators, differentiates to any order")
_SECOND_ORDER = (None, "cotangent", "complete")


def _primal(t):
    """``t`` without its forward-mode tangent (the reverse-mode graph stays)."""
    return torch.autograd.forward_ad.unpack_dual(t).primal


def _has_tangent(t):
    return torch.autograd.forward_ad.unpack_dual(t).tangent is not None


def _poison(x):
    """The gradient the cotangent-path Functions return for ``x``: NaN in ``x``'s shape, one scalar expanded.  The curvature
    term d/dx (v^T J(x)^T g) is not built, and a silent zero there would be a wrong number."""
    return torch.full((), float("nan"), device=x.device, dtype=x.dtype).expand(x.shape)


def _vjp_call(layer, x, aux, g):
    """``cvf_align_feature_vjp``: ``gx = J(x)^T g`` on the forward's aux rows, in ``x``'s shape."""
    B = x.shape[0]
    gx = torch.empty_like(x)
    if B > 0:
        g = g.to(device=x.device, dtype=torch.float32).contiguous()
        with torch.cuda.device(x.device):
            _hip.check(_hip.lib().cvf_align_feature_vjp(layer.pp_desc(), _hip.ptr(x), B, _hip.ptr(aux), _hip.ptr(g),
                                                        _hip.ptr(gx), _hip.stream()), "cvf_align_feature_vjp")
    return gx


def _jvp_call(layer, x, aux, v):
    """``cvf_align_feature_jvp``: ``q = J(x) v`` on the forward's aux rows, ``[B, d_r]``."""
    B = x.shape[0]
    q = torch.empty(B, layer.d_r, device=x.device, dtype=torch.float32)
    if B > 0:
        v = v.to(device=x.device, dtype=torch.float32).reshape(x.shape).contiguous()
        with torch.cuda.device(x.device):
            _hip.check(_hip.lib().cvf_align_feature_jvp(layer.pp_desc(), _hip.ptr(x), B, _hip.ptr(aux), _hip.ptr(v),
                                                        _hip.ptr(q), _hip.stream()), "cvf_align_feature_jvp")
    return q


def _hvp_call(layer, x, aux, g, v):
    """``cvf_align_feature_hvp``: ``h = d/dx <g, J(x) v>`` on the forward's aux rows, in ``x``'s shape."""
    B = x.shape[0]
    h = torch.empty_like(x)
    if B > 0:
        g = g.to(device=x.device, dtype=torch.float32).contiguous()
        v = v.to(device=x.device, dtype=torch.float32).reshape(x.shape).contiguous()
        with torch.cuda.device(x.device):
            _hip.check(_hip.lib().cvf_align_feature_hvp(layer.pp_desc(), _hip.ptr(x), B, _hip.ptr(aux), _hip.ptr(g), _hip.ptr(v),
                                                        _hip.ptr(h), _hip.stream()), "cvf_align_feature_hvp")
    return h


def _curvature(layer, g, v, x, aux):
    """What the cotangent-path Functions return for ``x``: ``d/dx <g, J(x) v>`` under ``second_order="complete"``, else NaN."""
    if layer.second_order == "complete":
        return _AlignHvpFn.apply(g, v, x, aux, layer)
    return _poison(x)


class _AlignFeatureFn(torch.autograd.Function):
    """``r(x)`` with its first derivative: forward = ``cvf_align_feature_fwd`` (features as rows, plus the per-frame aux rows
    R / centroid / Kinv), backward = ``cvf_align_feature_vjp`` on those aux rows, jvp (forward-mode AD) =
    ``cvf_align_feature_jvp`` on them.  ``x``: fp32, contiguous, on the layer's GPU.

    With ``layer.second_order`` set (``"cotangent"`` / ``"complete"``) the backward is itself a graph node (:class:`_AlignVjpFn`)."""

    @staticmethod
    def forward(ctx, x, layer):
        dev, B = x.device, x.shape[0]
        out = torch.empty(B, layer.d_r, device=dev, dtype=torch.float32)
        aux = torch.empty(_hip.ntiles(B), _hip.AUX_ROWS, _hip.TILE, device=dev, dtype=torch.float32)   # padded frame count
        if B > 0:
            with torch.cuda.device(dev):
                desc = layer.pp_desc()
                scratch = _hip.align_scratch(desc, B, dev)
                _hip.check(_hip.lib().cvf_align_feature_fwd(desc, _hip.ptr(x), B, None, _hip.ptr(out), _hip.ptr(aux),
                                                            _hip.ptr(scratch), _hip.stream()), "cvf_align_feature_fwd")
        ctx.save_for_backward(x, aux)
        ctx.save_for_forward(x, aux)
        ctx.layer = layer
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, aux = ctx.saved_tensors
        if ctx.layer.second_order is not None:
            return _AlignVjpFn.apply(grad_out, x, aux, ctx.layer), None
        if torch.is_grad_enabled():
            raise RuntimeError(_NO_DOUBLE_BACKWARD)
        return _vjp_call(ctx.layer, x, aux, grad_out), None

    @staticmethod
    def jvp(ctx, x_t, _):
        x, aux = ctx.saved_tensors
        return _AlignJvpFn.apply(x_t, _primal(x), aux, ctx.layer)


class _AlignVjpFn(torch.autograd.Function):
    """``(g, x, aux) -> gx = J(x)^T g`` as a graph node (``second_order="cotangent"`` / ``"complete"``).  Linear in ``g``: its
    backward returns ``J(x) v`` for ``g`` (:class:`_AlignJvpFn`, whose backward is this Function again - the pair is closed under
    any order of differentiation in ``g`` / ``v``).  For ``x`` it returns the curvature term ``d/dx <g, J(x) v>``
    (:class:`_AlignHvpFn`) under ``"complete"`` and NaN under ``"cotangent"``, where that term is left out.  Its jvp (forward
    mode over the backward) is ``J(x)^T g_t + d/dx <g, J(x) x_t>``."""

    @staticmethod
    def forward(ctx, g, x, aux, layer):
        ctx.save_for_backward(x, aux, g)
        ctx.save_for_forward(x, aux, g)
        ctx.layer = layer
        return _vjp_call(layer, x, aux, g)

    @staticmethod
    def backward(ctx, v):
        x, aux, g = ctx.saved_tensors
        q = _AlignJvpFn.apply(v, x, aux, ctx.layer) if ctx.needs_input_grad[0] else None
        return q, (_curvature(ctx.layer, g, v, x, aux) if ctx.needs_input_grad[1] else None), None, None

    @staticmethod
    def jvp(ctx, g_t, x_t, _aux_t, _):
        x, aux, g = (_primal(t) for t in ctx.saved_tensors)
        out = _AlignVjpFn.apply(g_t, x, aux, ctx.layer) if g_t is not None else None
        if x_t is not None:
            if ctx.layer.second_order != "complete":
                raise RuntimeError(_NO_DOUBLE_BACKWARD)
            h = _AlignHvpFn.apply(g, x_t, x, aux, ctx.layer)
            out = h if out is None else out + h
        return out


class _AlignJvpFn(torch.autograd.Function):
    """``(v, x, aux) -> q = J(x) v`` as a graph node: the tangent of forward-mode AD through the layer and the derivative of
    :class:`_AlignVjpFn` in its cotangent.  Its backward returns ``J(x)^T g`` for ``v``; for ``x`` the curvature term
    ``d/dx <g, J(x) v>`` under ``second_order="complete"``, else NaN."""

    @staticmethod
    def forward(ctx, v, x, aux, layer):
        ctx.save_for_backward(x, aux, v)
        ctx.layer = layer
        return _jvp_call(layer, x, aux, v)

    @staticmethod
    def backward(ctx, g):
        x, aux, v = ctx.saved_tensors
        gx = _AlignVjpFn.apply(g, x, aux, ctx.layer) if ctx.needs_input_grad[0] else None
        return gx, (_curvature(ctx.layer, g, v, x, aux) if ctx.needs_input_grad[1] else None), None, None


class _AlignHvpFn(torch.autograd.Function):
    """``(g, v, x, aux) -> h = d/dx <g, J(x) v>`` (``cvf_align_feature_hvp``): the curvature term of the layer's second
    derivative under ``second_order="complete"``.  Third derivatives are not built: its backward raises."""

    @staticmethod
    def forward(ctx, g, v, x, aux, layer):
        return _hvp_call(layer, x, aux, g, v)

    @staticmethod
    def backward(ctx, _):
        raise RuntimeError(_NO_THIRD_ORDER)


class FeatureLayer:
    """``FeatureLayer(feature_list, input_atom_group, use_angle_value=False)`` (main.ipynb:337)."""

    def __init__(self, feature_list, input_atom_group, use_angle_value=False):
        self.feature_list = list(feature_list)
        self.input_ix = _ix(input_atom_group)
        self.use_angle_value = use_angle_value
        lut = {int(g): i for i, g in enumerate(self.input_ix)}
        self.local = []
        for f in self.feature_list:
            try:
                self.local.append((f.type_name, tuple(lut[int(g)] for g in f.atom_indices)))
            except KeyError as e:
                raise ValueError(f"feature '{f.name}' uses atom {e} that is not in the input atom group") from None

    def get_feature_info(self):
        import pandas as pd
        # molann prints 1-based atom ids in this table (main.ipynb:306-307)
        return pd.DataFrame({"name": [f.name for f in self.feature_list], "type": [f.type_name for f in self.feature_list],
                             "type_id": [f.type_id for f in self.feature_list],
                             "atom indices": [list(f.atom_indices + 1) for f in self.feature_list]})

    def output_dimension(self):
        return sum(3 * len(a) if t == "position" else (2 if t == "dihedral" and not self.use_angle_value else 1)
                   for t, a in self.local)


class AlignmentLayer:
    """``AlignmentLayer(align_atom_group, input_atom_group)`` (main.ipynb:345)."""

    def __init__(self, align_atom_group, input_atom_group, weights=None, weights_any_size=False):
        self.weights = None if weights is None else np.asarray(weights, dtype=np.float64)
        self.weights_any_size = bool(weights_any_size)   # (AlignFeatureLayer: weighted layers of more than 64 atoms, opt-in)
        self.align_ix = _ix(align_atom_group)
        self.input_ix = _ix(input_atom_group)
        lut = {int(g): i for i, g in enumerate(self.input_ix)}
        try:
            self.local_idx = np.asarray([lut[int(g)] for g in self.align_ix], dtype=np.int64)
        except KeyError as e:
            raise ValueError(f"align atom {e} is not in the input atom group") from None
        pos = np.asarray(align_atom_group.positions, dtype=np.float64)
        self.ref_c = pos - pos.mean(axis=0, keepdims=True)   # (the fused layer re-centres by the weighted centroid)

    def show_info(self):
        print(f"\n{len(self.input_ix)} atoms used for input, (0-based) global indices: \n {list(self.input_ix)}")
        print(f"\n{len(self.align_ix)} atoms used for alignment, with (0-based) global indices: \n {list(self.align_ix)}")
        print("local indices\n", list(self.local_idx))
        print("\npositions of reference state used in aligment:\n", self.ref_c.astype(np.float32))


class PreprocessingANN(AlignFeatureLayer):
    """``PreprocessingANN(align_layer, feature_layer)`` (main.ipynb:348) -> one fused GPU layer."""

    def __init__(self, align_layer, feature_layer):
        if align_layer is None:   # molann: no alignment, the features of the raw coordinates
            AlignFeatureLayer.__init__(self, len(feature_layer.input_ix), None, None, feature_layer.local, feature_layer.use_angle_value)
            return
        assert np.array_equal(align_layer.input_ix, feature_layer.input_ix), "align and feature layers use different input atoms"
        super().__init__(len(align_layer.input_ix), align_layer.local_idx, align_layer.ref_c, feature_layer.local,
                         feature_layer.use_angle_value, align_weights=getattr(align_layer, "weights", None),
                         weights_any_size=getattr(align_layer, "weights_any_size", False))


def identity_desc(n_coord):
    d = _hip.PPDesc()
    d.mode, d.n_coord, d.d_r = _hip.PP_IDENTITY, int(n_coord), int(n_coord)
    return d


def factored_desc(d_r, rho):
    """Descriptor of CVF_PP_FACTORED records ``[r (d_r) | L (d_r x rho)]`` (include/cvf.h)."""
    d = _hip.PPDesc()
    d.mode, d.n_coord, d.d_r = _hip.PP_FACTORED, int(d_r) * (1 + int(rho)), int(d_r)
    return d


class FactoredMetric:
    """Per-frame records of an arbitrary preprocessing module for the generator loss (include/cvf.h, CVF_PP_FACTORED).

    The reference differentiates through ``pp_layer`` at every step (core.py:418-426).  Neither the module (never trained:
    the optimiser takes ``model.parameters()`` only, core.py:164-166) nor the frames change, so everything the step needs from
    the module is computed once per frame: the features ``r(x)`` and a factor ``L`` of the feature-space metric
    ``M(x) = J A J^T`` (``J = dr/dx``, ``d_r x n``; ``A = diag(diag_coeff)``), ``M = L L^T``:

    * ``n <= d_r``: ``L = J diag(sqrt(a))`` (``rho = n`` columns, exact);
    * ``n > d_r``: ``M`` in fp64, ``L = V diag(sqrt(max(lambda, 0)))`` from ``eigh(M)`` (``rho = d_r``).

    ``J`` is taken on a float64 deep copy of the module when the copy runs in fp64 (else on an fp32 copy); ``M`` and ``L`` are
    formed in fp64 and stored fp32.  The caller's module is never modified.

    Args:
        module: any ``torch.nn.Module`` mapping ``[B, *frame_shape]`` to ``[B, d_r]``, frame by frame.
        frame_shape: shape of one frame (``n = prod(frame_shape)`` floats, the reference's ``tot_dim``).
        diag_coeff: ``[n]`` non-negative coefficients, or None (ones).
        device: where the records are built and kept.
        probe: two or more frames for the checks (frame-locality of the module, output shape).
    """

    def __init__(self, module, frame_shape, diag_coeff, device, probe):
        self.frame_shape = tuple(int(v) for v in frame_shape)
        self.n = int(np.prod(self.frame_shape))
        self.device = torch.device(device)
        if diag_coeff is None:
            a = torch.ones(self.n, dtype=torch.float64)
        else:
            a = torch.as_tensor(diag_coeff).detach().to(device="cpu", dtype=torch.float64).reshape(-1)
        if a.numel() != self.n:
            raise ValueError(f"diag_coeff has {a.numel()} entries, the frames have {self.n} coordinates")
        if bool((a < 0).any()) or not bool(torch.isfinite(a).all()):
            raise ValueError("diag_coeff entries must be finite and >= 0 (A = diag(diag_coeff) is a metric)")
        self._sqrt_a = a.sqrt().to(self.device)
        self._a = a.to(self.device)
        X0 = torch.as_tensor(np.asarray(probe) if not torch.is_tensor(probe) else probe).to(self.device)
        if X0.shape[0] == 1:
            X0 = torch.cat([X0, X0 + 0.01], 0)
        X0 = X0[:2].reshape((2,) + self.frame_shape)
        try:   # fp64 when the module runs in fp64 (parameters, buffers and operators), else fp32
            self.module, self.dtype = copy.deepcopy(module).to(torch.float64), torch.float64
            X = X0.to(torch.float64)
            with torch.no_grad():
                y = self.module(X)
        except Exception:
            self.module, self.dtype = copy.deepcopy(module).to(torch.float32), torch.float32
            X = X0.to(torch.float32)
            with torch.no_grad():
                y = self.module(X)
        if y.dim() != 2 or y.shape[0] != 2:
            raise ValueError(f"the preprocessing module must map [B, {', '.join(map(str, self.frame_shape))}] to [B, d_r]; "
                             f"it returned shape {tuple(y.shape)} for two frames (1-D or 3-D outputs are not taken)")
        self.d_r = int(y.shape[1])
        self.rho = min(self.n, self.d_r)
        self.width = self.d_r * (1 + self.rho)
        # frame-locality: the reference's autograd.grad(y.sum(), X) (core.py:418-424) silently assumes that frame b's features
        # depend on frame b alone; a module that mixes frames (batch statistics, say) has no per-frame metric
        Jp = torch.autograd.functional.jacobian(lambda x: self.module(x), X).reshape(2, self.d_r, 2, self.n)
        if not bool(torch.isfinite(Jp).all()):
            raise ValueError("the preprocessing module's Jacobian is not finite on the first two frames of the trajectory")
        if bool((Jp[0, :, 1] != 0).any()) or bool((Jp[1, :, 0] != 0).any()):
            raise ValueError("the preprocessing module is not frame-local: features of one frame depend on another frame "
                             "of the batch (e.g. batch statistics); the generator loss needs a per-frame Jacobian")

    def record_bytes(self, n_frames):
        return int(n_frames) * self.width * 4

    def _chunk(self):
        per = 8 * self.d_r * (self.n + self.d_r) * 3 + 8 * self.n * 4   # J, M / L and their temporaries per frame, fp64
        return max(1, min(8192, (256 << 20) // per))

    def jacobian(self, X):
        """``(r, J)`` of the frames ``X`` ``[B, *frame_shape]`` in the builder's precision: ``[B, d_r]``, ``[B, d_r, n]``."""
        X = X.detach().to(device=self.device, dtype=self.dtype).reshape((-1,) + self.frame_shape).requires_grad_(True)
        with torch.enable_grad():
            y = self.module(X)
            J = torch.empty(X.shape[0], self.d_r, self.n, device=self.device, dtype=self.dtype)
            for i in range(self.d_r):
                g, = torch.autograd.grad(y[:, i].sum(), X, retain_graph=i + 1 < self.d_r, allow_unused=True)
                J[:, i] = 0.0 if g is None else g.reshape(X.shape[0], self.n)
        return y.detach(), J

    def factor(self, J):
        """``L`` (fp64, ``[B, d_r, rho]``) with ``L L^T = J A J^T``."""
        J = J.to(torch.float64)
        if self.n <= self.d_r:
            return J * self._sqrt_a
        M = torch.einsum("bin,n,bjn->bij", J, self._a, J)
        M = 0.5 * (M + M.transpose(1, 2))
        lam, V = torch.linalg.eigh(M)
        return V * lam.clamp_min(0.0).sqrt().unsqueeze(1)

    def records(self, frames, out=None):
        """fp32 records ``[B, d_r * (1 + rho)]`` of the frames (host or device array ``[B, *frame_shape]``), on the device,
        built ``_chunk()`` frames at a time (``out``: a preallocated destination)."""
        frames = torch.as_tensor(np.asarray(frames) if not torch.is_tensor(frames) else frames)
        B = frames.shape[0]
        if out is None:
            out = torch.empty(B, self.width, device=self.device, dtype=torch.float32)
        c = self._chunk()
        for s0 in range(0, B, c):
            r, J = self.jacobian(frames[s0:s0 + c].to(self.device))
            L = self.factor(J)
            out[s0:s0 + c, :self.d_r] = r.to(torch.float32)
            out[s0:s0 + c, self.d_r:] = L.reshape(L.shape[0], -1).to(torch.float32)
        return out

    def desc(self):
        return factored_desc(self.d_r, self.rho)


def module_features(module, frames, d_r, device, chunk=65536):
    """``module(frames)`` as fp32 rows ``[B, d_r]`` on the device, in chunks, without autograd (the transfer-operator loss and the
    autoencoders need the features only)."""
    frames = torch.as_tensor(np.asarray(frames) if not torch.is_tensor(frames) else frames)
    B = frames.shape[0]
    out = torch.empty(B, d_r, device=device, dtype=torch.float32)
    with torch.no_grad():
        for s0 in range(0, B, chunk):
            out[s0:s0 + chunk] = module(frames[s0:s0 + chunk].to(device=device, dtype=torch.float32)).reshape(-1, d_r)
    return out
