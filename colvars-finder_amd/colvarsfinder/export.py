"""TorchScript export of the collective-variable model (reference ``save_model``, core.py:205-226).

The reference scripts ``colvar_model() = Sequential(pp_layer, nets)`` and saves ``scripted_cv_cpu.pt`` /
``scripted_cv_gpu.pt`` for downstream programs (e.g. MD engines evaluating the learned CV through libtorch).
The training path of this package runs the alignment + feature layer as a gfx950 kernel behind a C ABI, which
TorchScript cannot serialise; :class:`ScriptableAlignFeature` is its *export twin*: the same map written with
torch operators only, so that the saved file is self-contained and runs wherever libtorch runs.

It is an export artefact, not a fallback: nothing in the training or evaluation path of this package
instantiates it (``save_model`` builds it for scripting and discards it).  Conventions as in ``pp.py``:
unweighted centroid of the align atoms, ``x_aligned = (x - c) @ R`` with
``R = U diag(1, 1, sign det(U V^T)) V^T`` from the SVD of ``(x_align - c)^T ref_c``; features in list order.
"""

from typing import List

import torch

from . import _hip


class ScriptableAlignFeature(torch.nn.Module):
    """Pure-torch, TorchScript-compatible alignment + feature map built from an ``AlignFeatureLayer``."""

    def __init__(self, layer):
        super().__init__()
        rec = layer.rec.detach().cpu().to(torch.long)
        self.d_r: int = int(layer.d_r)
        self.use_angle_value: bool = bool(layer.use_angle_value)
        # a layer without alignment (pp.PreprocessingANN(None, ...)): position records are the raw coordinates
        self.aligned: bool = bool(getattr(layer, "aligned", True))
        self.register_buffer("align_idx", layer.align_idx.detach().cpu().to(torch.long))
        self.register_buffer("ref_c", layer.ref_c.detach().cpu().clone())
        # per-atom alignment weights (mean 1; ref_c is already multiplied by them, pp.AlignFeatureLayer); ones = uniform
        aw = getattr(layer, "align_w", None)
        self.register_buffer("align_w", torch.ones(layer.ref_c.shape[0]) if aw is None else aw.detach().cpu().clone())

        def pick(type_id, n_atoms):
            rows = rec[rec[:, 0] == type_id]
            return rows[:, 1:1 + n_atoms].contiguous(), rows[:, 5].contiguous()

        pos_a, pos_o = pick(_hip.FEAT_POSITION, 1)
        bond_a, bond_o = pick(_hip.FEAT_BOND, 2)
        ang_a, ang_o = pick(_hip.FEAT_ANGLE, 3)
        dih_a, dih_o = pick(_hip.FEAT_DIHEDRAL, 4)
        self.register_buffer("pos_atoms", pos_a.reshape(-1))
        self.register_buffer("pos_out", (pos_o[:, None] + torch.arange(3)[None, :]).reshape(-1))
        self.register_buffer("bond_atoms", bond_a)
        self.register_buffer("bond_out", bond_o)
        self.register_buffer("ang_atoms", ang_a)
        self.register_buffer("ang_out", ang_o)
        self.register_buffer("dih_atoms", dih_a)
        self.register_buffer("dih_out", dih_o)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        ref = self.ref_c.to(x.dtype)
        out = torch.zeros(x.shape[0], self.d_r, dtype=x.dtype, device=x.device)
        if self.pos_atoms.numel() > 0 and not self.aligned:
            out[:, self.pos_out] = x[:, self.pos_atoms, :].reshape(x.shape[0], -1)
        if self.pos_atoms.numel() > 0 and self.aligned:
            xa = x[:, self.align_idx, :]
            c = (self.align_w.to(x.dtype)[None, :, None] * xa).mean(dim=1, keepdim=True)
            h = torch.matmul((xa - c).transpose(1, 2), ref)
            u, s, vh = torch.linalg.svd(h)
            d = torch.sign(torch.linalg.det(torch.matmul(u, vh)))
            ones = torch.ones_like(d)
            r = torch.matmul(u * torch.stack([ones, ones, d], dim=-1)[:, None, :], vh)
            al = torch.matmul(x[:, self.pos_atoms, :] - c, r)
            out[:, self.pos_out] = al.reshape(x.shape[0], -1)
        if self.bond_out.numel() > 0:
            d01 = x[:, self.bond_atoms[:, 1], :] - x[:, self.bond_atoms[:, 0], :]
            out[:, self.bond_out] = torch.sqrt((d01 * d01).sum(-1))
        if self.ang_out.numel() > 0:
            r1 = x[:, self.ang_atoms[:, 0], :] - x[:, self.ang_atoms[:, 1], :]
            r2 = x[:, self.ang_atoms[:, 2], :] - x[:, self.ang_atoms[:, 1], :]
            cs = (r1 * r2).sum(-1) / torch.sqrt((r1 * r1).sum(-1) * (r2 * r2).sum(-1))
            out[:, self.ang_out] = torch.acos(cs) if self.use_angle_value else cs
        if self.dih_out.numel() > 0:
            b1 = x[:, self.dih_atoms[:, 1], :] - x[:, self.dih_atoms[:, 0], :]
            b2 = x[:, self.dih_atoms[:, 2], :] - x[:, self.dih_atoms[:, 1], :]
            b3 = x[:, self.dih_atoms[:, 3], :] - x[:, self.dih_atoms[:, 2], :]
            n1 = torch.cross(b1, b2, dim=-1)
            n2 = torch.cross(b2, b3, dim=-1)
            inv = 1.0 / torch.sqrt((n1 * n1).sum(-1) * (n2 * n2).sum(-1))
            cs = (n1 * n2).sum(-1) * inv
            sn = (n1 * b3).sum(-1) * torch.sqrt((b2 * b2).sum(-1)) * inv
            if self.use_angle_value:
                out[:, self.dih_out] = torch.atan2(sn, cs)
            else:
                out[:, self.dih_out] = cs
                out[:, self.dih_out + 1] = sn
        return out


def scriptable_cv(cv: torch.nn.Sequential) -> torch.nn.Sequential:
    """``colvar_model()`` with a kernel-backed preprocessing layer replaced by its export twin (deep copies on CPU)."""
    import copy
    mods: List[torch.nn.Module] = []
    for m in cv.children():
        if hasattr(m, "pp_desc") and hasattr(m, "rec"):
            mods.append(ScriptableAlignFeature(m))
        else:
            mods.append(copy.deepcopy(m).to("cpu"))
    return torch.nn.Sequential(*mods)


# ------------------------------------------------------------------------------------------------------------------------
# The self-contained model file of a trained CV (include/cvf.h: cvf_cv_file_*) and its evaluator.
# TorchScript (save_model) serves programs that link libtorch; this file serves a C caller of libcvf_hip.so - an MD engine that
# needs xi(x) and grad_x xi(x) for one frame per step: cvf_cv_file_bind once, cvf_cv_frame_eval per step.
# ------------------------------------------------------------------------------------------------------------------------
CV_FILE_MAGIC, CV_FILE_VERSION, CV_FILE_DIR_OFFSET = b"CVF1", 1, 960
# table ids of the directory (include/cvf.h: CVF_FILE_*), element type 0 = int32, 1 = float32
CV_FILE_TABLES = (("align_idx", 1, 0), ("ref_c", 2, 1), ("rec", 3, 0), ("align_w", 4, 1), ("atom_align", 5, 0), ("atom_slot", 6, 0),
                  ("rec_slot", 7, 0), ("slot_atom", 8, 0), ("mrec", 9, 0), ("slot_row", 10, 0), ("theta", 11, 1))


def _cv_parts(cv):
    """``(pp scalars dict, tables dict of CPU numpy arrays, MLPDesc, upto_layer, k, n_shared)`` of a ``colvar_model()`` /
    ``reg_model()`` (``n_shared > 0``: form C, under ``cv.shared_trunk = True``)."""
    import numpy as np
    from .pp import AlignFeatureLayer
    if not hasattr(cv, "_pp_and_nets"):
        raise NotImplementedError(f"save_cv_file takes what colvar_model() returns, got a {type(cv).__name__}")
    pp, nets = cv._pp_and_nets()
    if not isinstance(pp, (torch.nn.Identity, AlignFeatureLayer)):
        raise NotImplementedError(f"the preprocessing layer is a {type(pp).__name__}: a CV file holds an Identity or an "
                                  "AlignFeatureLayer (a foreign pp_layer has no tables to write)")
    try:
        desc, upto, k, params, n_shared = cv._plan(nets)
    except TypeError as e:
        raise NotImplementedError(str(e)) from e
    theta = torch.cat([p.detach().to(device="cpu", dtype=torch.float32).reshape(-1) for p in params]).numpy()
    i32, f32 = (lambda t: np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.int32).reshape(-1)), \
               (lambda t: np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32).reshape(-1))
    empty_i, empty_f = np.zeros(0, np.int32), np.zeros(0, np.float32)
    if isinstance(pp, torch.nn.Identity):
        n = int(desc.dims[0])
        sc = dict(mode=_hip.PP_IDENTITY, n_coord=n, n_align=0, n_rec=0, d_r=n, use_angle_value=0, has_position=0, flags=0,
                  n_slot=0, n_rec_slot=0, n_mrec=0, n_ref=0)
        tabs = {name: (empty_f if ty else empty_i) for name, _, ty in CV_FILE_TABLES}
    else:
        with_rows = pp._n_ref < 65536 and pp._n_slot < 65536 and getattr(pp, "_row_off_max", 0) < 256   # as pp_desc()
        sc = dict(mode=_hip.PP_ALIGN if pp.aligned else _hip.PP_FEATURES, n_coord=3 * pp.n_atoms, n_align=int(pp.align_idx.numel()),
                  n_rec=int(pp.rec.shape[0]), d_r=int(pp.d_r), use_angle_value=int(pp.use_angle_value),
                  has_position=int(bool((pp.rec[:, 0] == _hip.FEAT_POSITION).any().item())), flags=int(pp._flags),
                  n_slot=int(pp._n_slot), n_rec_slot=int(pp._n_rec_slot), n_mrec=int(pp.mrec.shape[0]) if with_rows else 0,
                  n_ref=int(pp._n_ref) if with_rows else 0)
        tabs = dict(align_idx=i32(pp.align_idx), ref_c=f32(pp.ref_c) if pp.aligned else empty_f, rec=i32(pp.rec),
                    align_w=f32(pp.align_w) if pp.align_w is not None else empty_f, atom_align=i32(pp.atom_align),
                    atom_slot=i32(pp.atom_slot), rec_slot=i32(pp.rec_slot), slot_atom=i32(pp.slot_atom),
                    mrec=i32(pp.mrec) if with_rows else empty_i, slot_row=i32(pp.slot_row) if with_rows else empty_i)
    tabs["theta"] = theta
    return sc, tabs, desc, int(upto), int(k), int(n_shared)


def cv_file_bytes(cv) -> bytes:
    """The bytes :func:`save_cv_file` writes (layout: include/cvf.h, ``cvf_cv_file_*``)."""
    import struct
    sc, tabs, desc, upto, k, n_shared = _cv_parts(cv)
    head = CV_FILE_MAGIC + struct.pack("<3i", CV_FILE_VERSION, _hip.MAX_NETS, _hip.MAX_LAYERS) + bytes(desc)
    head += struct.pack("<12i", *(sc[f] for f in ("mode", "n_coord", "n_align", "n_rec", "d_r", "use_angle_value", "has_position",
                                                  "flags", "n_slot", "n_rec_slot", "n_mrec", "n_ref")))
    head += struct.pack("<4i", upto, k, len(CV_FILE_TABLES), n_shared)
    assert len(head) == CV_FILE_DIR_OFFSET
    pos = (CV_FILE_DIR_OFFSET + 24 * len(CV_FILE_TABLES) + 15) // 16 * 16
    directory, body = b"", b""
    data_off = pos
    for name, tid, ty in CV_FILE_TABLES:
        a = tabs[name]
        directory += struct.pack("<2i2q", tid, ty, a.size, pos if a.size else 0)
        if a.size:
            raw = a.astype("<f4" if ty else "<i4", copy=False).tobytes()
            body += raw + b"\0" * (-len(raw) % 16)
            pos += len(raw) + (-len(raw) % 16)
    blob = head + directory
    return blob + b"\0" * (data_off - len(blob)) + body


def save_cv_file(cv, path):
    """Write ``colvar_model()`` as ONE self-contained little-endian file a C caller binds with ``cvf_cv_file_bind`` and evaluates
    with ``cvf_cv_frame_eval`` - the nets' flat parameters and description and ALL tables of the preprocessing layer, so that the
    bound model also feeds the three-call recipe.  ``NotImplementedError`` (with the reason) for models the HIP nets' kernels do
    not describe: a ``RegModel`` without ``shared_trunk``, foreign modules, a foreign ``pp_layer``.  With ``cv.shared_trunk = True``
    a ``SharedEigenFunctions`` model and the ``RegModel`` of ``reg_model()`` are written in form C (``n_shared > 0`` at byte 956,
    ``theta`` with the trunk once; a C caller asks ``cvf_cv_file_n_shared`` and evaluates with ``cvf_cv_frame_shared_eval``).
    ``save_model`` and its TorchScript files are a different artefact and are not touched."""
    blob = cv_file_bytes(cv)
    with open(path, "wb") as f:
        f.write(blob)
    return path


class FrameCV:
    """``xi(x)`` and ``d xi / d x`` of a saved (path) or live (``colvar_model()``) CV on the kernels a C caller of the file gets.

    Both forms go through the file's bytes and ``cvf_cv_file_bind`` into one torch-owned device buffer.  ``fc(X, coef=None)``
    returns ``(xi [B, k], J [B, k, *frame])`` or, with ``coef [B, k]``, ``(xi, F [B, *frame])`` with
    ``F = sum_i coef_i d xi_i / d x`` (the bias force up to sign), on ``X``'s device and in its floating-point type, like
    ``jacobian()``.  ``fc.supported`` is ``(bool, reason)`` of ``cvf_cv_frame_supported``; ``fc.route`` is ``"frame"`` (one
    launch, one wave per frame: ``cvf_cv_frame_eval``) or ``"three-call"`` (``cvf_align_feature_fwd`` -> ``cvf_cv_nets_eval`` ->
    ``cvf_align_feature_vjp_rows`` on the same bound model: large molecules, wide nets).  The one launch is built for one frame
    or a few replicas per call; DESIGN.md section 4.15 gives the batch size above which the three-call recipe is the faster of
    the two (``jacobian()`` is that recipe for whole trajectories).

    ``large_frames=True`` opts into the one launch for frames of any size (``cvf_cv_frame_large_eval``, one workgroup per frame;
    DESIGN.md section 4.16): the route is ``"frame"`` where the wave kernel takes the model, else ``"frame-large"`` where
    ``cvf_cv_frame_large_supported`` does, else ``"three-call"``.  ``fc.supported_large`` is ``(bool, reason)`` of that predicate
    (asked with or without the option; ``fc.supported`` keeps its meaning).  Section 4.16 gives the measured times of both routes
    and the batch size at which they meet; the default stays ``False``.

    ``fc.n_shared`` is the file's ``n_shared`` (``cvf_cv_file_n_shared``).  With ``n_shared > 0`` (form C, DESIGN.md section
    4.17) the predicates and launches are the ``_shared`` ones and the three-call recipe runs ``cvf_cv_nets_shared_eval``;
    ``route``, ``supported`` and ``supported_large`` keep their meaning."""

    _infix = ""   # the one-launch entry points are cvf_cv_frame[_large]<_infix>[_shared]_supported / _eval (BiasedCV: "_bias")

    def __init__(self, path_or_cv, device="cuda", large_frames=False):
        import ctypes as C
        if isinstance(path_or_cv, (str, bytes)) or hasattr(path_or_cv, "__fspath__"):
            with open(path_or_cv, "rb") as f:
                blob = f.read()
        else:
            blob = cv_file_bytes(path_or_cv)
        self.device = _hip.require_gpu(torch.device(device))
        lib = _hip.lib()
        need = lib.cvf_cv_file_device_bytes(blob, len(blob))
        if need <= 0:
            raise ValueError(f"not a CV file ({need}): {lib.cvf_last_error().decode()}")
        with torch.cuda.device(self.device):
            self._buf = torch.empty(need, device=self.device, dtype=torch.uint8)
            self.model = _hip.CVModel()
            _hip.check(lib.cvf_cv_file_bind(blob, len(blob), C.c_void_p(self._buf.data_ptr()), need, C.byref(self.model),
                                            _hip.stream()), "cvf_cv_file_bind")
        self.k, self.n_coord, self.d_r = int(self.model.k), int(self.model.pp.n_coord), int(self.model.pp.d_r)
        self.n_shared = int(lib.cvf_cv_file_n_shared(blob, len(blob)))
        # form C: the _shared entry points take n_shared where their namesakes take upto_layer
        sh = self.n_shared > 0
        self._cut = self.n_shared if sh else int(self.model.upto_layer)
        entry = lambda large, what: getattr(lib, "cvf_cv_frame" + large + self._infix + ("_shared" if sh else "") + what)
        self._frame_eval, self._large_eval = entry("", "_eval"), entry("_large", "_eval")
        self._nets_scratch = lib.cvf_cv_nets_shared_scratch_floats if sh else lib.cvf_cv_nets_scratch_floats
        self._nets_eval = lib.cvf_cv_nets_shared_eval if sh else lib.cvf_cv_nets_eval
        frame_ok, large_ok = entry("", "_supported"), entry("_large", "_supported")
        ok = frame_ok(C.byref(self.model.mlp), self._cut, C.byref(self.model.pp)) == 1
        self.supported = (ok, None if ok else lib.cvf_last_error().decode())
        ok_large = large_ok(C.byref(self.model.mlp), self._cut, C.byref(self.model.pp)) == 1
        self.supported_large = (ok_large, None if ok_large else lib.cvf_last_error().decode())
        self.route = "frame" if ok else ("frame-large" if large_frames and ok_large else "three-call")

    def __call__(self, X, coef=None):
        import ctypes as C
        import numpy as np
        X = torch.as_tensor(np.asarray(X) if not torch.is_tensor(X) else X)
        src_dev, src_dt = X.device, (X.dtype if X.dtype.is_floating_point else torch.float32)
        B, frame_shape = int(X.shape[0]), tuple(X.shape[1:])
        assert int(np.prod(frame_shape)) == self.n_coord, f"frames have {int(np.prod(frame_shape))} coordinates, the model takes {self.n_coord}"
        dev, k, n = self.device, self.k, self.n_coord
        lib, P, m = _hip.lib(), _hip.ptr, self.model
        with torch.cuda.device(dev):
            s = _hip.stream()
            x = X.detach().to(device=dev, dtype=torch.float32).reshape(B, n).contiguous()
            cf = None
            if coef is not None:
                cf = torch.as_tensor(coef).detach().to(device=dev, dtype=torch.float32).reshape(B, k).contiguous()
            xi = torch.empty(B, k, device=dev, dtype=torch.float32)
            D = torch.empty((B, n) if cf is not None else (B, k, n), device=dev, dtype=torch.float32)
            if B > 0 and self.route == "frame":
                _hip.check(self._frame_eval(C.byref(m.mlp), C.c_void_p(m.theta), self._cut, C.byref(m.pp), P(x), B, P(cf),
                                            P(xi), P(D), s), self._frame_eval.__name__)
            elif B > 0 and self.route == "frame-large":
                _hip.check(self._large_eval(C.byref(m.mlp), C.c_void_p(m.theta), self._cut, C.byref(m.pp), P(x), B, P(cf),
                                            P(xi), P(D), s), self._large_eval.__name__)
            elif B > 0:
                self._three_call(x, cf, xi, D, s)
        D = D.reshape(((B,) if cf is not None else (B, k)) + frame_shape)
        return xi.to(device=src_dev, dtype=src_dt), D.to(device=src_dev, dtype=src_dt)

    def _three_call(self, x, cf, xi, D, s):
        """cvf_align_feature_fwd -> cvf_cv_nets_eval (form C: cvf_cv_nets_shared_eval) -> cvf_align_feature_vjp[_rows] on the bound model."""
        import ctypes as C
        lib, P, m, dev = _hip.lib(), _hip.ptr, self.model, self.device
        B, k, d_r, T = int(x.shape[0]), self.k, self.d_r, _hip.ntiles(int(x.shape[0]))
        pp, mlp, theta = C.byref(m.pp), C.byref(m.mlp), C.c_void_p(m.theta)
        r = r_t = aux = None
        if m.pp.mode == _hip.PP_IDENTITY:
            r = x
        else:
            r_t = torch.empty(T, d_r, _hip.TILE, device=dev, dtype=torch.float32)
            aux = torch.empty(T, _hip.AUX_ROWS, _hip.TILE, device=dev, dtype=torch.float32)
            scratch = _hip.align_scratch(m.pp, B, dev)
            _hip.check(lib.cvf_align_feature_fwd(pp, P(x), B, P(r_t), None, P(aux), P(scratch), s), "cvf_align_feature_fwd")
        G = torch.empty(B, k, d_r, device=dev, dtype=torch.float32)
        ws = torch.empty(self._nets_scratch(mlp, self._cut, B, 1), device=dev, dtype=torch.float32)
        _hip.check(self._nets_eval(mlp, theta, self._cut, P(r), P(r_t), B, P(xi), P(G), None, P(ws), s), self._nets_eval.__name__)
        if cf is None:
            _hip.check(lib.cvf_align_feature_vjp_rows(pp, P(x), B, P(aux), k, P(G), P(D), s), "cvf_align_feature_vjp_rows")
        else:   # the contraction at the feature level (k terms per feature), then one coordinate pass
            g = torch.einsum("bk,bkr->br", cf, G).contiguous()
            _hip.check(lib.cvf_align_feature_vjp(pp, P(x), B, P(aux), P(g), P(D), s), "cvf_align_feature_vjp")


# ------------------------------------------------------------------------------------------------------------------------
# Bias energy and forces along the CV in one launch, in an MD engine's arrays (include/cvf.h: cvf_cv_*_bias_*)
# ------------------------------------------------------------------------------------------------------------------------
def bias_desc(terms, k, device=None):
    """``(BiasDesc, table)`` of a list of bias terms on ``k`` CVs, checked with ``cvf_cv_bias_check`` (``ValueError`` with the C
    message).  A term is a dict or a tuple in the vocabulary of ``cvf_bias_desc``:

    ``{"kind": "harmonic" | "upper_wall" | "lower_wall", "cv": i, "kappa": .., "center": ..}`` or ``(kind, i, kappa, center)``;
    ``{"kind": "linear", "cv": i, "kappa": ..}`` or ``("linear", i, kappa)``;
    ``{"kind": "table", "cv": i, "lo": .., "inv_h": .. (or "h": spacing), "u": U at the nodes, "du": U' at the nodes}`` or
    ``("table", i, lo, h, u, du)``;
    ``{"kind": "table2d", "cv": i, "cv2": j, "lo": (a, b), "h": (h1, h2) (or "inv_h": ..), "u", "d1", "d2", "d12": arrays [n1, n2]}``:
    a joint grid ``U(xi_i, xi_j)`` of bicubic Hermite cells.  Both table kinds take ``"n": (n1, n2)``
    (``"n": n1`` for ``"table"``) in place of the arrays: a zero-filled grid to deposit hills into (:meth:`BiasedCV.deposit`).

    ``table`` is the fp32 tensor (on ``device``; ``None`` without table terms) of all nodes' ``(U_j, U'_j)`` pairs - of a 2-D term
    the four floats ``(U, d1 U, d2 U, d12 U)`` per node, ``j2`` fastest, from a multiple of 4 floats on - that
    ``BiasDesc.table`` points to; term ``t``'s nodes start at ``desc.term[t].tab_off``.  ``device=None`` keeps it on the CPU
    (for checks without a GPU: the pointer is then a host pointer, which no launch may take)."""
    import numpy as np
    d = _hip.BiasDesc()
    d.n_terms = len(terms)
    pairs = []
    n_table = 0
    for t, term in enumerate(terms[:_hip.BIAS_MAX_TERMS]):
        if not isinstance(term, dict):
            kind = term[0]
            keys = ("kind", "cv", "kappa") if kind == "linear" else ("kind", "cv", "lo", "h", "u", "du") if kind == "table" \
                else ("kind", "cv", "kappa", "center")
            if len(term) != len(keys):
                raise ValueError(f"bias term {t}: a {kind!r} tuple is {keys}, got {len(term)} entries")
            term = dict(zip(keys, term))
        kind = term["kind"]
        two_d = kind == "table2d"
        if two_d:
            kind = "table"
        if isinstance(kind, str):
            if kind not in _hip.BIAS_KINDS:
                raise ValueError(f"bias term {t}: kind {kind!r} is none of {sorted(_hip.BIAS_KINDS) + ['table2d']}")
            kind = _hip.BIAS_KINDS[kind]
        e = d.term[t]
        e.kind, e.cv = int(kind), int(term["cv"])
        if two_d:
            if "n" in term:
                n1, n2 = (int(v) for v in term["n"])
                nodes = np.zeros((n1, n2, 4), dtype=np.float32)
            else:
                four = [np.asarray(term[key], dtype=np.float32) for key in ("u", "d1", "d2", "d12")]
                if four[0].ndim != 2 or any(a.shape != four[0].shape for a in four):
                    raise ValueError(f"bias term {t}: u, d1, d2 and d12 are arrays [n1, n2] of one shape, got {[a.shape for a in four]}")
                nodes = np.stack(four, axis=2)
            (e.lo, e.lo2), e.cv2 = (float(v) for v in term["lo"]), int(term["cv2"])
            e.inv_h, e.inv_h2 = (float(v) for v in term["inv_h"]) if "inv_h" in term else (1.0 / float(v) for v in term["h"])
            if n_table % 4:    # a 2-D node is one 16-byte access
                pairs.append(np.zeros(4 - n_table % 4, dtype=np.float32))
                n_table += 4 - n_table % 4
            e.tab_off, e.n_nodes, e.n_nodes2 = n_table, int(nodes.shape[0]), int(nodes.shape[1])
            pairs.append(nodes.reshape(-1))
            n_table += nodes.size
        elif kind == _hip.BIAS_TABLE:
            if "n" in term:
                u = du = np.zeros(int(term["n"]), dtype=np.float32)
            else:
                u, du = np.asarray(term["u"], dtype=np.float32).reshape(-1), np.asarray(term["du"], dtype=np.float32).reshape(-1)
            if u.shape != du.shape:
                raise ValueError(f"bias term {t}: {u.size} values of U and {du.size} of U' at the nodes")
            e.lo = float(term["lo"])
            e.inv_h = float(term["inv_h"]) if "inv_h" in term else 1.0 / float(term["h"])
            e.tab_off, e.n_nodes = n_table, int(u.size)
            pairs.append(np.stack([u, du], axis=1).reshape(-1))
            n_table += 2 * int(u.size)
        else:
            e.kappa, e.center = float(term["kappa"]), float(term.get("center", 0.0))
    d.n_table = n_table
    table = None
    if pairs:
        table = torch.empty(n_table, dtype=torch.float32, device="cpu" if device is None else device)   # (torch's own, aligned storage)
        table.copy_(torch.from_numpy(np.concatenate(pairs)))
        d.table = table.data_ptr()
    if _hip.lib().cvf_cv_bias_check(d, int(k)) != 1:
        raise ValueError(_hip.lib().cvf_last_error().decode())
    return d, table


def _table2d_torch(e, table, a, b):
    """``(U, dU/da, dU/db)`` of a joint grid term at ``(a, b)``: cvf_bias_term2_eval of csrc/cvf_bias.hpp with torch operators."""
    n1, n2 = e.n_nodes, e.n_nodes2
    nodes = table[e.tab_off:e.tab_off + 4 * n1 * n2].to(device=a.device, dtype=a.dtype).reshape(n1, n2, 4)

    def axis(x, lo, inv_h, n):
        s = (x - lo) * inv_h
        below, above = ~(s >= 0), s > n - 1
        j = torch.nan_to_num(s.detach(), nan=0.0).clamp(0, n - 2).floor().long()
        w = torch.where(below, torch.zeros_like(s), torch.where(above, torch.ones_like(s), s - j))
        d = torch.where(below, x - lo, torch.where(above, (s - (n - 1)) * (1.0 / inv_h), torch.zeros_like(s)))
        return j, w, d

    def hermite(w, h, inv_h, u0, d0, u1, d1, diff=None):
        w2, w3 = w * w, w * w * w
        diff = u0 - u1 if diff is None else diff       # (taken between neighbouring nodes: inv_h magnifies what it has lost)
        v = (2.0 * w3 - 3.0 * w2 + 1.0) * u0 + (3.0 * w2 - 2.0 * w3) * u1 + h * ((w3 - 2.0 * w2 + w) * d0 + (w3 - w2) * d1)
        dv = inv_h * (6.0 * (w2 - w) * diff) + (3.0 * w2 - 4.0 * w + 1.0) * d0 + (3.0 * w2 - 2.0 * w) * d1
        return v, dv

    j1, x, e1 = axis(a, e.lo, e.inv_h, n1)
    j2, y, e2 = axis(b, e.lo2, e.inv_h2, n2)
    h1, h2 = 1.0 / e.inv_h, 1.0 / e.inv_h2
    c = [[nodes[j1 + i, j2 + j] for j in (0, 1)] for i in (0, 1)]      # the cell's corners
    line = []
    for i in (0, 1):     # on node line j1 + i: (U, d2 U) and (d1 U, d12 U) along cv2
        line.append(hermite(y, h2, e.inv_h2, c[i][0][:, 0], c[i][0][:, 2], c[i][1][:, 0], c[i][1][:, 2])
                    + hermite(y, h2, e.inv_h2, c[i][0][:, 1], c[i][0][:, 3], c[i][1][:, 1], c[i][1][:, 3]))
    (p0, q0, r0, s0), (p1, q1, r1, s1) = line
    pd, qd = hermite(y, h2, e.inv_h2, c[0][0][:, 0] - c[1][0][:, 0], c[0][0][:, 2] - c[1][0][:, 2], c[0][1][:, 0] - c[1][1][:, 0],
                     c[0][1][:, 2] - c[1][1][:, 2])          # p0 - p1 and q0 - q1 from the corner differences
    U, U1 = hermite(x, h1, e.inv_h, p0, r0, p1, r1, pd)
    U2, U12 = hermite(x, h1, e.inv_h, q0, s0, q1, s1, qd)
    return U + U1 * e1 + U2 * e2 + U12 * (e1 * e2), U1 + U12 * e2, U2 + U12 * e1


def bias_torch(desc, table, xi):
    """``(U [B], dU [B, k])`` of ``xi [B, k]`` by the term formulas of csrc/cvf_bias.hpp written with torch operators in ``xi``'s
    type and on its device, the table read now - what ``BiasedCV``'s ``"three-call"`` route evaluates in fp32."""
    U, dU = torch.zeros_like(xi[:, 0]), torch.zeros_like(xi)
    zero = torch.zeros_like(xi[:, 0])
    for t in range(desc.n_terms):
        e = desc.term[t]
        x = xi[:, e.cv]
        d = x - e.center
        if e.kind == _hip.BIAS_LINEAR:
            u, du = e.kappa * x, e.kappa + zero
        elif e.kind == _hip.BIAS_TABLE and e.n_nodes2 != 0:
            u, du, du2 = _table2d_torch(e, table, x, xi[:, e.cv2])
            dU[:, e.cv2] = dU[:, e.cv2] + du2
        elif e.kind == _hip.BIAS_TABLE:
            nodes = table[e.tab_off:e.tab_off + 2 * e.n_nodes].to(device=xi.device, dtype=xi.dtype).reshape(-1, 2)
            last, h = e.n_nodes - 1, 1.0 / e.inv_h
            s = (x - e.lo) * e.inv_h
            j = s.detach().clamp(0, last - 1).floor().long()
            w = s - j
            w2, w3 = w * w, w * w * w
            u0, d0, u1, d1 = nodes[j, 0], nodes[j, 1], nodes[j + 1, 0], nodes[j + 1, 1]
            g00 = 6.0 * (w2 - w)
            u = (2.0 * w3 - 3.0 * w2 + 1.0) * u0 + (3.0 * w2 - 2.0 * w3) * u1 + h * ((w3 - 2.0 * w2 + w) * d0 + (w3 - w2) * d1)
            du = e.inv_h * (g00 * (u0 - u1)) + (3.0 * w2 - 4.0 * w + 1.0) * d0 + (3.0 * w2 - 2.0 * w) * d1
            below, above = ~(s >= 0), s > last
            u = torch.where(below, nodes[0, 0] + nodes[0, 1] * (x - e.lo), torch.where(above, nodes[last, 0] + nodes[last, 1] * ((s - last) * h), u))
            du = torch.where(below, nodes[0, 1] + zero, torch.where(above, nodes[last, 1] + zero, du))
        else:
            on = torch.ones_like(x, dtype=torch.bool) if e.kind == _hip.BIAS_HARMONIC else (x > e.center if e.kind == _hip.BIAS_UPPER_WALL else x < e.center)
            u, du = torch.where(on, 0.5 * e.kappa * d * d, zero), torch.where(on, e.kappa * d, zero)
        U = U + u
        dU[:, e.cv] = dU[:, e.cv] + du
    return U, dU


class BiasedCV(FrameCV):
    """Bias energy and forces along a saved (path) or live (``colvar_model()``) CV, accumulated into an MD engine's force array
    in ONE launch (``cvf_cv_frame_bias_eval`` and its ``_large`` / ``_shared`` forms).

    The model is bound as :class:`FrameCV` binds it.  ``terms`` is the bias (:func:`bias_desc`); ``bc.table`` is the device
    tensor of all table nodes that the launch reads AT LAUNCH TIME - update it in place (metadynamics, ABF) and the next call
    sees it.  ``atom_index`` (no repeats; ``None`` = the identity) and ``atom_stride`` say where the CV's ``n_coord / 3`` atoms
    lie in the engine's arrays: atom ``a`` of frame ``b`` is ``X_all[b].reshape(-1)[atom_index[a] * atom_stride + c]``.

    ``bc(X_all, F_all)`` takes float32 device tensors ``[B, ...]`` whose frames are contiguous (a frame stride larger than the
    frame is fine: slice a larger tensor), ADDS ``- sum_t U_t'(xi) d xi / d x`` to ``F_all`` in place - only the CV's atoms'
    three floats are touched - and returns ``(xi [B, k], U [B], dU [B, k])``, ``dU[b, i] = sum_{t: cv = i} U_t'(xi_i)``.

    ``bc.route`` is ``"frame"`` (one wave per frame), ``"frame-large"`` (``large_frames=True``, one workgroup per frame) or
    ``"three-call"``: ``FrameCV``'s recipe for all k gradient rows, the same term formulas in torch fp32 (:func:`bias_torch`)
    and one contraction - several launches, the same result up to rounding (another summation order, torch's own elementwise
    arithmetic), for the models the one launch declines.

    Periodic cells: ``bc(X_all, F_all, cell=cell)`` takes the engine's WRAPPED positions and makes the CV's
    atoms whole inside the launch, along the order of ``atom_index`` (atom j takes the image nearest to the whole atom j - 1: consecutive
    atoms must lie closer than half the shortest cell height).  ``cell`` is a float32 device tensor ``[9]``, ``[3, 3]`` (one cell for
    all frames) or ``[B, 9]``, ``[B, 3, 3]``, the lattice vectors as rows in lower-triangular form, read AT LAUNCH TIME (a barostat
    rescales it in place; an axis with a diagonal entry <= 0 is not periodic).  ``virial=V`` (float32 device ``[B, 9]`` or ``[B, 3, 3]``)
    is filled with ``V[b, i, j] = sum_a r_a[i] f_a[j]`` over the whole positions and the force just added; it is also taken without
    a cell, for positions that are whole already.  ``bc.route_cell`` is the route such a call takes (the workgroup launch keeps 4
    more bytes of LDS per atom).  With ``cell is None and virial is None`` the call is the one above, bit for bit.

    ``bc.deposit(xi, height, sigma, ...)`` adds metadynamics hills to a table term of ``bc.table`` on the device, from the ``xi`` a
    call returned; a ``"table"`` or ``"table2d"`` term given by ``"n"`` starts as a zero-filled grid."""

    _infix = "_bias"

    def __init__(self, path_or_cv, terms, device="cuda", large_frames=False, atom_index=None, atom_stride=3):
        device = torch.device(device)
        if device.type == "cuda" and device.index is None and torch.cuda.is_available():   # (the engine's tensors are compared with it)
            device = torch.device("cuda", torch.cuda.current_device())
        super().__init__(path_or_cv, device=device, large_frames=large_frames)   # (binds; route and supported from the bias predicates)
        self._bias_eval = {"frame": self._frame_eval, "frame-large": self._large_eval}
        # the same with a periodic cell and / or the virial (the _cell entry points; their limits differ by the image counts' LDS)
        import ctypes as C
        lib, sh = _hip.lib(), "_shared" if self.n_shared > 0 else ""
        self._cell_eval = {"frame": getattr(lib, f"cvf_cv_frame_bias{sh}_cell_eval"), "frame-large": getattr(lib, f"cvf_cv_frame_large_bias{sh}_cell_eval")}
        m = self.model
        ok = getattr(lib, f"cvf_cv_frame_bias{sh}_cell_supported")(C.byref(m.mlp), self._cut, C.byref(m.pp)) == 1
        self.supported_cell = (ok, None if ok else lib.cvf_last_error().decode())
        ok_large = getattr(lib, f"cvf_cv_frame_large_bias{sh}_cell_supported")(C.byref(m.mlp), self._cut, C.byref(m.pp)) == 1
        self.supported_large_cell = (ok_large, None if ok_large else lib.cvf_last_error().decode())
        self.route_cell = "frame" if ok else ("frame-large" if large_frames and ok_large else "three-call")
        with torch.cuda.device(self.device):
            self.desc, self.table = bias_desc(terms, self.k, self.device)
        self.atom_stride = int(atom_stride)
        if self.atom_stride < 3:
            raise ValueError(f"atom_stride = {atom_stride}: an atom has at least 3 floats")
        self.atom_index = None
        if atom_index is not None:
            if self.n_coord % 3 != 0:
                raise ValueError(f"atom_index with n_coord = {self.n_coord}: an atom index needs frames of whole atoms")
            idx = torch.as_tensor(atom_index).reshape(-1).to(torch.int64).cpu()
            if idx.numel() != self.n_coord // 3 or (idx < 0).any() or idx.unique().numel() != idx.numel():
                raise ValueError(f"atom_index: {self.n_coord // 3} distinct non-negative atom numbers are needed "
                                 f"(got {idx.numel()}, {idx.unique().numel()} distinct, min {int(idx.min()) if idx.numel() else 0})")
            self.atom_index = idx.to(device=self.device, dtype=torch.int32)
        a = torch.arange(self.n_coord, device=self.device)
        at = a // 3 if self.atom_index is None else self.atom_index.long()[a // 3]
        self._cols = at * self.atom_stride + a % 3            # float of coordinate j inside a frame
        self._extent = int(self._cols.max()) + 1

    def _frames(self, T, name):
        if not (torch.is_tensor(T) and T.dtype == torch.float32 and T.device == self.device and T.dim() >= 2):
            raise ValueError(f"{name} must be a float32 tensor [B, ...] on {self.device}")
        B = int(T.shape[0])
        per = int(T[0].numel()) if B else 0
        try:
            V = T.view(B, per)      # (frames contiguous inside; any stride between them)
        except RuntimeError as e:
            raise ValueError(f"{name}: the frames must be contiguous ({e})") from e
        if B and per < self._extent:
            raise ValueError(f"{name}: frames of {per} floats, the CV's atoms reach float {self._extent - 1}")
        return V, B, (int(V.stride(0)) if B > 1 else per)

    def _cell_args(self, cell, virial, B):
        """(cell tensor or None, its frame stride, virial tensor [B, 9] or None) of a call's ``cell`` and ``virial``."""
        if self.n_coord % 3 != 0:
            raise ValueError(f"cell / virial with n_coord = {self.n_coord}: a cell and a virial need frames of whole atoms")
        stride = 0
        if cell is not None:
            cell = torch.as_tensor(cell).to(device=self.device, dtype=torch.float32)
            if cell.numel() == 9:
                cell = cell.reshape(9)
            elif cell.numel() == 9 * B and cell.shape[0] == B:
                cell, stride = cell.reshape(B, 9), 9
            else:
                raise ValueError(f"cell: [9], [3, 3], [{B}, 9] or [{B}, 3, 3] floats are needed, got {tuple(cell.shape)}")
            cell = cell.contiguous()
        if virial is not None:
            if not (torch.is_tensor(virial) and virial.dtype == torch.float32 and virial.device == self.device and virial.is_contiguous()
                    and virial.numel() == 9 * B and (B == 0 or virial.shape[0] == B)):
                raise ValueError(f"virial must be a contiguous float32 tensor [{B}, 9] or [{B}, 3, 3] on {self.device}")
        return cell, stride, virial

    def __call__(self, X_all, F_all, cell=None, virial=None):
        import ctypes as C
        Xv, B, xs = self._frames(X_all, "X_all")
        Fv, Bf, fs = self._frames(F_all, "F_all")
        if B != Bf:
            raise ValueError(f"X_all has {B} frames, F_all {Bf}")
        if cell is not None or virial is not None:
            return self._call_cell(Xv, Fv, B, xs, fs, *self._cell_args(cell, virial, B))
        lib, m, k, dev = _hip.lib(), self.model, self.k, self.device
        with torch.cuda.device(dev):
            s = _hip.stream()
            xi, U, dU = (torch.empty(B, k, device=dev), torch.empty(B, device=dev), torch.empty(B, k, device=dev))
            if B == 0:
                return xi, U, dU
            if self.route in self._bias_eval:
                lay = _hip.MDLayout(self.atom_index.data_ptr() if self.atom_index is not None else None, self.atom_stride, 0, xs, fs)
                fn = self._bias_eval[self.route]
                _hip.check(fn(C.byref(m.mlp), C.c_void_p(m.theta), self._cut, C.byref(m.pp), C.byref(self.desc), C.byref(lay),
                              C.c_void_p(Xv.data_ptr()), B, _hip.ptr(xi), _hip.ptr(U), _hip.ptr(dU), C.c_void_p(Fv.data_ptr()), s),
                           fn.__name__)
            else:
                x = Xv[:, self._cols].contiguous()
                D = torch.empty(B, k, self.n_coord, device=dev)
                self._three_call(x, None, xi, D, s)
                U, dU = bias_torch(self.desc, self.table, xi)
                Fv[:, self._cols] -= torch.einsum("bk,bkn->bn", dU, D)
        return xi, U, dU

    def _call_cell(self, Xv, Fv, B, xs, fs, cell, cell_stride, virial):
        """The call with a periodic cell and / or the virial, on ``self.route_cell``."""
        import ctypes as C
        lib, m, k, dev = _hip.lib(), self.model, self.k, self.device
        with torch.cuda.device(dev):
            s = _hip.stream()
            xi, U, dU = (torch.empty(B, k, device=dev), torch.empty(B, device=dev), torch.empty(B, k, device=dev))
            if B == 0:
                return xi, U, dU
            lay = _hip.MDLayout(self.atom_index.data_ptr() if self.atom_index is not None else None, self.atom_stride, 0, xs, fs)
            mc = _hip.MDCell(cell.data_ptr() if cell is not None else None, cell_stride, virial.data_ptr() if virial is not None else None)
            if self.route_cell in self._cell_eval:
                fn = self._cell_eval[self.route_cell]
                _hip.check(fn(C.byref(m.mlp), C.c_void_p(m.theta), self._cut, C.byref(m.pp), C.byref(self.desc), C.byref(lay),
                              C.c_void_p(Xv.data_ptr()), B, _hip.ptr(xi), _hip.ptr(U), _hip.ptr(dU), C.c_void_p(Fv.data_ptr()), s, C.byref(mc)),
                           fn.__name__)
            else:     # cvf_md_make_whole (the gather and the chain in one launch), the three calls, the virial from the dense arrays
                if cell is not None:
                    x = torch.empty(B, self.n_coord, device=dev)
                    _hip.check(lib.cvf_md_make_whole(C.byref(lay), C.byref(mc), C.c_void_p(Xv.data_ptr()), self.n_coord // 3, B, _hip.ptr(x), s),
                               "cvf_md_make_whole")
                else:
                    x = Xv[:, self._cols].contiguous()
                D = torch.empty(B, k, self.n_coord, device=dev)
                self._three_call(x, None, xi, D, s)
                U, dU = bias_torch(self.desc, self.table, xi)
                f = -torch.einsum("bk,bkn->bn", dU, D)
                Fv[:, self._cols] += f
                if virial is not None:
                    virial.view(B, 3, 3).copy_(torch.einsum("bai,baj->bij", x.view(B, -1, 3), f.view(B, -1, 3)))
        return xi, U, dU

    def deposit(self, xi, height, sigma, term=None, bias_factor=None, kT=None):
        """Add one Gaussian hill per row of ``xi [B, k]`` (float32 on the device - what a call just returned) to a table term, in
        ``bc.table``, on the device (``cvf_cv_bias_deposit``): the next call sees it, on every route.

        ``sigma`` is the width, ``(sigma1, sigma2)`` for a ``"table2d"`` term; ``term`` the index of the table term (``None``: the
        only one).  ``bias_factor`` and ``kT`` together make the deposit well-tempered, ``w = height exp(-V / ((bias_factor - 1)
        kT))`` with ``V`` the term's own value at the centre before this call.  Returns ``hills [B, 4] = (c1, c2, w, V)``."""
        import ctypes as C
        tables = [t for t in range(self.desc.n_terms) if self.desc.term[t].kind == _hip.BIAS_TABLE]
        if term is None:
            if len(tables) != 1:
                raise ValueError(f"term=None needs exactly one table term, the bias has {len(tables)}: name one of {tables}")
            term = tables[0]
        if (bias_factor is None) != (kT is None):
            raise ValueError("bias_factor and kT go together (well-tempered) or are both left out (plain metadynamics)")
        inv_kdt = 0.0 if kT is None else 1.0 / ((float(bias_factor) - 1.0) * float(kT))
        s1, s2 = (float(v) for v in sigma) if hasattr(sigma, "__len__") else (float(sigma), 0.0)
        if not (torch.is_tensor(xi) and xi.dtype == torch.float32 and xi.device == self.device and xi.dim() == 2 and xi.shape[1] == self.k):
            raise ValueError(f"xi must be a float32 tensor [B, {self.k}] on {self.device}")
        xi = xi.contiguous()
        B = int(xi.shape[0])
        hill = _hip.HillDesc(int(term), 0, float(height), s1, s2, inv_kdt)
        with torch.cuda.device(self.device):
            hills = torch.empty(B, 4, device=self.device)
            rc = _hip.lib().cvf_cv_bias_deposit(C.byref(self.desc), self.k, C.byref(hill), _hip.ptr(xi), B, _hip.ptr(self.table),
                                                _hip.ptr(hills), _hip.stream())
        if rc == -1:
            raise ValueError(_hip.lib().cvf_last_error().decode())
        _hip.check(rc, "cvf_cv_bias_deposit")
        return hills


def make_whole(X, cell, atom_index=None, atom_stride=3, device="cuda"):
    """The atoms of wrapped frames made whole under a periodic cell, in one launch (``cvf_md_make_whole``; the rule of
    csrc/cvf_cell.hpp): atom 0 stays, atom j takes the periodic image nearest to the whole atom j - 1, in
    the order of ``atom_index`` (``None``: all atoms of a frame in their order).  For trajectories read from an engine's wrapped
    output before training, and what ``BiasedCV``'s ``"three-call"`` route runs first.

    ``X``: ``[B, ...]`` frames whose atoms are ``atom_stride`` floats apart (array or tensor; a float32 tensor on the device is read
    in place, frames contiguous inside); ``cell``: ``[9]`` / ``[3, 3]`` for all frames or ``[B, 9]`` / ``[B, 3, 3]``, lattice vectors as
    rows, lower-triangular (an axis with a diagonal entry <= 0 or not finite is not periodic).  Consecutive atoms must lie closer
    than half the shortest cell height.  Returns the dense float32 device tensor ``[B, n_atoms, 3]``.

    ``device`` (beyond the plain ``make_whole(X, cell, atom_index, atom_stride)``): where host arrays are taken to and the launch
    runs; leave it at its default unless several GPUs are in use.  ``atom_index`` is range-checked on the host against the frame
    size, so an index that is a device tensor costs one copy back and a synchronisation per call - pass a list or a CPU tensor in
    a loop."""
    import ctypes as C
    import numpy as np
    device = _hip.require_gpu(device)
    X = torch.as_tensor(np.asarray(X) if not torch.is_tensor(X) else X).detach().to(device=device, dtype=torch.float32)
    if X.dim() < 2:
        raise ValueError("X must be [B, ...] frames")
    B = int(X.shape[0])
    per = int(X[0].numel()) if B else 0
    try:
        Xv = X.view(B, per)
    except RuntimeError:
        Xv = X.reshape(B, per).contiguous()
    atom_stride = int(atom_stride)
    if atom_stride < 3:
        raise ValueError(f"atom_stride = {atom_stride}: an atom has at least 3 floats")
    idx = None
    if atom_index is not None:
        idx = torch.as_tensor(atom_index).reshape(-1).to(torch.int64).cpu()
        if idx.numel() < 1 or (idx < 0).any() or (B and int(idx.max()) * atom_stride + 3 > per):
            raise ValueError(f"atom_index: atom numbers inside frames of {per} floats are needed")
        n_atoms = int(idx.numel())
        idx = idx.to(device=device, dtype=torch.int32)
    else:
        n_atoms = (per - 3) // atom_stride + 1 if per >= 3 else 0
    cell = torch.as_tensor(np.asarray(cell) if not torch.is_tensor(cell) else cell).to(device=device, dtype=torch.float32)
    if cell.numel() == 9:
        cell, stride = cell.reshape(9).contiguous(), 0
    elif cell.numel() == 9 * B and cell.shape[0] == B:
        cell, stride = cell.reshape(B, 9).contiguous(), 9
    else:
        raise ValueError(f"cell: [9], [3, 3], [{B}, 9] or [{B}, 3, 3] floats are needed, got {tuple(cell.shape)}")
    out = torch.empty(B, n_atoms, 3, device=device, dtype=torch.float32)
    if B == 0 or n_atoms == 0:
        return out
    with torch.cuda.device(device):
        lay = _hip.MDLayout(idx.data_ptr() if idx is not None else None, atom_stride, 0, int(Xv.stride(0)) if B > 1 else per, 0)
        mc = _hip.MDCell(cell.data_ptr(), stride, None)
        _hip.check(_hip.lib().cvf_md_make_whole(C.byref(lay), C.byref(mc), C.c_void_p(Xv.data_ptr()), n_atoms, B, _hip.ptr(out), _hip.stream()),
                   "cvf_md_make_whole")
    return out
