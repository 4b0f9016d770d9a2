"""Training tasks with the API of the reference's ``colvarsfinder.core`` on MI355X.

API twin (own code) of reference ``colvarsfinder/core.py``: ``TrainingTask`` (core.py:60-249),
``EigenFunctionTask`` (core.py:251-566) and ``AutoEncoderTask`` (core.py:569-744) keep their
constructor arguments, defaults, public methods and attributes, so the reference's example
scripts run unchanged (``device`` defaults to ``torch.device('cuda')``, PyTorch-ROCm's name for the HIP device; the
modules returned by ``colvar_model()`` / ``reg_model()`` take CPU tensors and answer on the CPU, as the notebooks'
evaluation cells expect).  What differs is *how* a
step is computed: the model's parameters live in one flat HBM buffer, the trajectory shard is
resident in HBM and pre-permuted once (batches are static: ``shuffle=False``, core.py:472-481),
and every step is a short sequence of hand-written gfx950 kernels called through the C ABI of
``libcvf_hip.so`` (``include/cvf.h``) - no autograd graph, no per-step host synchronisation.

Per-step pipeline of ``EigenFunctionTask`` (generator mode, core.py:418-426,438):
    K1  align + features           cvf_align_feature_fwd     replaces pp_layer(X)           core.py:403
    K4a nets forward + dY/dfeat    cvf_ef_mlp_fwd            replaces model(...)            core.py:403
    K2/3 q = J A J^T g, E          cvf_metric_apply          replaces autograd.grad x k     core.py:424-426
    K5  batch sums (fp64)          cvf_ef_stats              core.py:406-410,446-452
    C1  all-reduce of the sums     torch.distributed (RCCL)  (absent in the reference)
        scalar tail + d loss/d sum cvf_ef_loss               core.py:426-457
    K4b parameter gradient         cvf_ef_backward           replaces loss.backward()       core.py:517
    C2  all-reduce of the gradient torch.distributed (RCCL)
    K6  Adam                       cvf_adam_step             replaces optimizer.step()      core.py:522

There is no CPU path: ``device`` must be a HIP device (``torch.device('cuda')`` is PyTorch's name
for it) and the HIP extension must be built, otherwise construction raises.
"""

import copy
import gc
import math
import os
import types
from abc import ABC, abstractmethod
from typing import NamedTuple, Optional

import numpy as np
import pandas as pd
import torch

import ctypes

from . import _dist, _hip
from .nn import AutoEncoder, EigenFunctions, RegAutoEncoder, RegModel, SharedEigenFunctions, mlp_layout  # noqa: F401
from .nn import _strict_chain_layers
from .pp import AlignFeatureLayer, FactoredMetric, identity_desc, module_features

try:  # logging sink of the reference (core.py:50,143); optional here
    from tensorboardX import SummaryWriter as _SummaryWriter
except Exception:  # pragma: no cover - tensorboardX is not part of the image
    _SummaryWriter = None

try:
    from tqdm import tqdm as _tqdm
except Exception:  # pragma: no cover
    def _tqdm(it, **_):
        return it


def C_pointer(struct):
    return ctypes.pointer(struct)


class _ScalarLog:
    """Stand-in for ``tensorboardX.SummaryWriter`` when that package is absent: keeps the scalars."""

    def __init__(self, logdir=None):
        self.logdir, self.scalars = logdir, []

    def add_scalar(self, tag, value, step):
        self.scalars.append((tag, float(value), int(step)))


def _split(n, test_ratio):
    """Same draw as ``sklearn.model_selection.train_test_split`` at core.py:465,468,672: one permutation
    from NumPy's global RNG; test = first ceil(ratio n) entries, train = the rest."""
    n_test = int(math.ceil(test_ratio * n))
    perm = np.random.permutation(n)
    return perm[n_test:], perm[:n_test]


def _agreed_split(n, test_ratio, draws, device):
    """``(idx_train, idx_test)`` of the last of ``draws`` :func:`_split` calls (the eigenfunction task draws twice and keeps the
    second, core.py:465,468; the autoencoder tasks draw once, core.py:672,1044), every rank brought to rank 0's permutation."""
    for _ in range(draws):
        idx_train, idx_test = _split(n, test_ratio)
    if _dist.world() > 1:
        both = torch.as_tensor(np.concatenate([idx_train, idx_test]), device=device)
        _dist.broadcast_(both)
        both = both.cpu().numpy()
        idx_train, idx_test = both[:len(idx_train)], both[len(idx_train):]
    return idx_train, idx_test


def _static_batches(n, bs, rank=None, world=None):
    """The static batches of a permuted set of ``n`` frames - DataLoader(batch_size=bs, drop_last=True, shuffle=False),
    core.py:470-481 - as this process sees them: ``(pos, nb, ranges)``.  ``pos``: the positions (into the permuted set) it keeps
    resident - one process: the whole set, the tail that drop_last discards included; a data-parallel job: this rank's slice of
    every global batch, batch-major (_dist.shard_batches).  ``nb``: frames per local batch; ``ranges``: the batches as row ranges
    ``(a, b)`` of the resident rows.  No batch when ``bs == 0`` or ``n < bs``."""
    rank, world = _dist.rank() if rank is None else rank, _dist.world() if world is None else world
    # (each set by itself: a rank without steps would leave the others waiting)
    assert bs == 0 or bs >= world, f"batch size {bs} is smaller than the number of ranks {world}"
    pos, nb = _dist.shard_batches(n, bs, rank, world)
    ranges = [(j * nb, (j + 1) * nb) for j in range(len(pos) // nb)] if nb > 0 else []
    return (np.arange(n, dtype=np.int64) if world == 1 else pos), nb, ranges


def _batch_weight_sums(w, ranges):
    """Global weight sum of every batch ``w[a:b]`` as host floats: batches are static (shuffle=False), so their weight sums are
    known before the first step."""
    if not ranges:
        return []
    sums = torch.stack([w[a:b].sum(dtype=torch.float64) for a, b in ranges])
    _dist.allreduce_sum_(sums)
    return [float(v) for v in sums.cpu()]


class _AsyncEpochLog:
    """The per-epoch loss rows leave the device through a small ring of pinned buffers, asynchronously: the host side of an
    epoch (``loss_list``, ``_cvec``, the writer's scalars - ``on_epoch(epoch, train_rows, test_rows)``) runs up to
    ``depth - 1`` epochs later, in order, instead of draining the stream after every epoch (with a few steps per epoch that
    drain was most of the epoch: 1.38 -> 0.54 ms per epoch at config 3).  Epochs that save or plot ``flush_all()`` first."""

    def __init__(self, log_tr, log_te, n_tr, n_te, on_epoch, depth=4):
        self.log_tr, self.log_te, self.n_tr, self.n_te, self.on_epoch = log_tr, log_te, n_tr, n_te, on_epoch
        self.ring = [dict(tr=torch.zeros(log_tr.shape, dtype=log_tr.dtype).pin_memory(),
                          te=torch.zeros(log_te.shape, dtype=log_te.dtype).pin_memory(), ev=torch.cuda.Event(), pending=None)
                     for _ in range(depth)]

    def _flush(self, slot):
        slot["ev"].synchronize()
        _dist.check_comm()    # a cross-rank exchange that timed out has poisoned these rows with NaN: stop here, loudly
        ep, slot["pending"] = slot["pending"], None
        self.on_epoch(ep, slot["tr"][:self.n_tr].clone(), slot["te"][:self.n_te].clone())

    def reserve(self, epoch):
        """Finish the epoch that still occupies this epoch's ring slot (callers with side buffers of their own do this first)."""
        slot = self.ring[epoch % len(self.ring)]
        if slot["pending"] is not None:
            self._flush(slot)
        return slot

    def push(self, epoch):
        slot = self.reserve(epoch)
        slot["tr"][:self.n_tr].copy_(self.log_tr[:self.n_tr], non_blocking=True)
        slot["te"][:self.n_te].copy_(self.log_te[:self.n_te], non_blocking=True)
        slot["ev"].record()
        slot["pending"] = epoch

    def flush_all(self):
        for slot in sorted((s_ for s_ in self.ring if s_["pending"] is not None), key=lambda s_: s_["pending"]):
            self._flush(slot)


class _CVModel(torch.nn.Sequential):
    """What ``colvar_model()`` / ``reg_model()`` return: ``Sequential(preprocessing_layer, nets)`` as in the reference
    (core.py:372-382, 640-647, 855-877), evaluated on the task's GPU whatever device the input lives on.  The reference's
    callers pass CPU tensors made from the trajectory and call ``.detach().numpy()`` on the result (2d.ipynb:437-446,
    main.ipynb:561-562, and ``plot_class.plot(self.colvar_model(), ...)`` at core.py:530-532): the input is moved to the
    device, alignment kernel and nets run there, the result comes back on the input's device and floating-point type.

    ``shared_trunk`` (default ``False``; a settable attribute, ``cv.shared_trunk = True``) opts a model whose ``k`` chains share
    their first layers - a ``SharedEigenFunctions``, or the ``RegModel`` of ``reg_model()`` - into form C of the evaluation
    kernels (``cvf_cv_*_shared_*``): the trunk is described, stored and run once.  Then
    :meth:`nets_route` answers ``("hip", None)`` for both, :meth:`jacobian` / :meth:`metric_tensor` take
    ``cvf_cv_nets_shared_eval``, and ``export.save_cv_file`` / ``export.FrameCV`` write and evaluate the form-C file.  Models of
    every other type behave as with ``False``."""

    shared_trunk = False

    def __init__(self, *modules, device=None):
        super().__init__(*modules)
        self._cvf_device = None if device is None else torch.device(device)

    def _compute_device(self):
        if self._cvf_device is not None:
            return self._cvf_device
        for t in list(self.parameters()) + list(self.buffers()):   # (a slice of this Sequential: where its tensors live)
            return t.device
        return torch.device("cuda")

    def _autograd_twin(self):
        """The same map written with torch operators only (the alignment layer replaced by export.ScriptableAlignFeature, the
        nets as they are), on the compute device - what the reference's own ``Sequential`` is (core.py:372-382): used when the
        caller wants d xi / d x through autograd.  The HIP kernels carry no autograd graph."""
        from .export import ScriptableAlignFeature
        mods = []
        for m in self.children():
            mods.append(ScriptableAlignFeature(m).to(self._compute_device()) if hasattr(m, "pp_desc") and hasattr(m, "rec") else m)
        return torch.nn.Sequential(*mods)

    def forward(self, x):
        x = torch.as_tensor(x)
        dev = _hip.require_gpu(self._compute_device())
        src_dev, src_dt = x.device, (x.dtype if x.dtype.is_floating_point else torch.float32)
        if x.requires_grad and torch.is_grad_enabled():
            # differentiable call (the reference returns a plain differentiable Sequential: d xi / d x by autograd, e.g. for the
            # Dirichlet energy of a learned CV): torch operators on the GPU in fp32, graph attached, answer in the caller's type
            with torch.cuda.device(dev):
                out = self._autograd_twin()(x.to(device=dev, dtype=torch.float32))   # (the nets' parameters are fp32)
            return out.to(device=src_dev, dtype=src_dt)
        with torch.cuda.device(dev):
            out = super().forward(x.detach().to(device=dev, dtype=torch.float32))
        return out.to(device=src_dev, dtype=src_dt)

    # ---------------------------------------------------------------- derivatives of the CVs in the coordinates
    # share of the free device memory the default chunk's workspace may take
    JACOBIAN_MEMORY_FRACTION = 0.25

    def jacobian(self, X, chunk=None):
        """``(xi, J)`` of the frames ``X`` ``[B, *frame_shape]`` (CPU or device tensor or numpy array, fp32 or fp64):
        ``xi [B, k]`` and ``J [B, k, *frame_shape]``, ``J[b, i] = d xi_i / d x`` at frame ``b``, on ``X``'s device and in its
        floating-point type, without an autograd graph.  Columns follow the model's outputs (EigenFunctionTask: ``cvec``).

        ``Identity`` and ``AlignFeatureLayer`` preprocessing: the nets' part ``xi`` and ``d xi / d r`` by the per-layer HIP kernels
        of ``cvf_cv_nets_eval`` when the nets are an ``EigenFunctions`` or a ``create_sequential_nn`` chain such as an encoder
        (:meth:`nets_route`), by ``torch.func`` otherwise (fp32, on the device); the coordinate part by the HIP kernel
        ``cvf_align_feature_vjp_rows`` (all k rows of a frame in one pass).
        Any other preprocessing module, and alignment layers whose tables exceed the derivative kernels' limits
        (``AlignFeatureLayer.derivative_table_limits()``), take the slow route: torch autograd through the whole map, one
        backward per CV.  ``chunk`` bounds the device workspace in frames (default: from the free device memory)."""
        return self._derivatives(X, chunk, want_m=False)

    def metric_tensor(self, X, diag_coeff=None, chunk=None):
        """``(xi, M)``: ``M [B, k, k] = J A J^T`` per frame with ``J`` as in :meth:`jacobian` and ``A = diag(diag_coeff)``
        (``[tot_dim]``, non-negative and finite; ones by default) - the CV metric tensor (diffusion matrix of the effective
        dynamics along xi, and the per-frame form of the generator's Rayleigh quotient).  ``J`` is never formed on the HIP
        routes: ``q_j = J A J^T g_j`` comes from ``cvf_metric_apply`` (the generator step's kernel) and
        ``M_ij = g_i . q_j`` from ``cvf_metric_gram``.  Alignment layers past ``derivative_table_limits()`` raise
        ``NotImplementedError``; :meth:`jacobian` still takes them."""
        X = self._frames_in(X)
        tot_dim = int(np.prod(X.shape[1:]))
        a = self._check_diag_coeff(diag_coeff, tot_dim)
        return self._derivatives(X, chunk, want_m=True, a=a)

    @staticmethod
    def _frames_in(X):
        return torch.as_tensor(np.asarray(X) if not torch.is_tensor(X) else X)

    @staticmethod
    def _check_diag_coeff(diag_coeff, tot_dim):
        """``diag_coeff`` as an fp64 CPU vector of length ``tot_dim`` (None: ones); ValueError when it is not a metric."""
        if diag_coeff is None:
            return torch.ones(tot_dim, dtype=torch.float64)
        a = torch.as_tensor(np.asarray(diag_coeff) if not torch.is_tensor(diag_coeff) else diag_coeff)
        a = a.detach().to(device="cpu", dtype=torch.float64).reshape(-1)
        if a.numel() != tot_dim:
            raise ValueError(f"diag_coeff has {a.numel()} entries, the frames have {tot_dim} coordinates")
        if not bool(torch.isfinite(a).all()) or bool((a < 0).any()):
            raise ValueError("diag_coeff entries must be finite and >= 0 (A = diag(diag_coeff) is a metric)")
        return a

    def _pp_and_nets(self):
        mods = list(self.children())
        return mods[0], (mods[1] if len(mods) == 2 else torch.nn.Sequential(*mods[1:]))

    def nets_route(self):
        """``("hip", None)`` when :meth:`jacobian` / :meth:`metric_tensor` take the nets' part ``xi = nets(r)``, ``d xi / d r`` from
        ``cvf_cv_nets_eval`` (csrc/cv_nets.hip), ``("torch", reason)`` when they take it from ``torch.func``.  Decided from the
        model alone (no device is touched): the nets must be an ``EigenFunctions`` or a ``create_sequential_nn`` chain - Linear
        layers and activations the kernels implement - of a shape ``cvf_cv_nets_supported`` accepts, behind an ``Identity`` or an
        ``AlignFeatureLayer`` within its derivative tables' limits."""
        pp, nets = self._pp_and_nets()
        if not isinstance(pp, (torch.nn.Identity, AlignFeatureLayer)):
            return "torch", f"the preprocessing layer {type(pp).__name__} takes the slow route (torch autograd through the whole map)"
        if isinstance(pp, AlignFeatureLayer) and pp.derivative_table_limits() is not None:
            return "torch", f"the feature list has {pp.derivative_table_limits()}: the slow route"
        try:
            self._plan(nets)
        except TypeError as e:
            return "torch", str(e)
        return "hip", None

    _SHARED_HINT = ("; shared_trunk = True on the model (cv.shared_trunk = True) takes its trunk-and-heads form on HIP "
                    "(cvf_cv_nets_shared_eval)")

    def _plan(self, nets):
        """``(desc, upto_layer, k, params, n_shared)``: :meth:`_nets_plan_shared` for a trunk-and-heads model under
        ``shared_trunk = True``, else :meth:`_nets_plan` with ``n_shared = 0``.  TypeError with the reason."""
        if self.shared_trunk and type(nets) in (SharedEigenFunctions, RegModel):
            desc, L, k, params, ns = self._nets_plan_shared(nets)
            return desc, L, k, params, ns
        try:
            return self._nets_plan(nets) + (0,)
        except TypeError as e:
            if type(nets) is RegModel:
                raise TypeError(str(e) + self._SHARED_HINT) from None
            raise

    @staticmethod
    def _nets_plan_shared(nets):
        """``(desc, n_layers, k, params, n_shared)`` of form C (include/cvf.h: ``cvf_cv_nets_shared_eval``): ``k`` scalar chains
        whose first ``n_shared`` layers are one set of tensors, every tensor once in ``params`` (the trunk, then head 0, head
        1, ..) and the trunk's offsets the same for every net.  A ``SharedEigenFunctions`` gives ``n_shared = nets.n_shared``; a
        ``RegModel`` gives the chains ``encoder + reg[cvec[i]]`` in ``cvec`` order, ``n_shared`` = the encoder's Linear layers.
        TypeError with the reason for everything else.  Built from the modules on every call, like :meth:`_nets_plan`."""
        if type(nets) is SharedEigenFunctions:
            chains, ns = [_strict_chain_layers(net) for net in nets.eigen_funcs], int(nets.n_shared)
            if any(a[0] is not b[0] for c in chains for a, b in zip(c[:ns], chains[0][:ns])):
                raise TypeError(f"the first {ns} Linear layers of the eigenfunctions are not the same modules")
        elif type(nets) is RegModel:
            if nets.reg is None or len(nets.cvec) < 1:
                raise TypeError("the RegModel has no regulariser nets")
            trunk = _strict_chain_layers(nets.encoder)
            heads = [_strict_chain_layers(nets.reg[int(i)]) for i in nets.cvec]
            chains, ns = [trunk + h for h in heads], len(trunk)
            if trunk[-1][0].out_features != heads[0][0][0].in_features:
                raise TypeError(f"the encoder has {trunk[-1][0].out_features} outputs, the regulariser nets take {heads[0][0][0].in_features}")
        else:
            raise TypeError(f"the nets are a {type(nets).__name__}: cvf_cv_nets_shared_eval takes a SharedEigenFunctions or a RegModel")
        shape = lambda c: [(lin.in_features, lin.out_features, act) for lin, act in c]
        if any(shape(c) != shape(chains[0]) for c in chains):
            raise TypeError("the nets behind the trunk differ in architecture")
        L, k = len(chains[0]), len(chains)
        if not 1 <= k <= _hip.MAX_NETS:
            raise TypeError(f"k = {k} nets: the kernels take 1 to {_hip.MAX_NETS}")
        if L > _hip.MAX_LAYERS:
            raise TypeError(f"{L} layers: the kernels take 1 to {_hip.MAX_LAYERS}")
        if chains[0][-1][0].out_features != 1:
            raise TypeError(f"the nets behind the trunk must be scalar (they have {chains[0][-1][0].out_features} outputs each)")
        d, params, pos = _hip.MLPDesc(), [], 0
        d.n_nets, d.n_layers = k, L
        for l, (fin, fout, act) in enumerate(shape(chains[0])):
            d.dims[l], d.dims[l + 1], d.act[l] = fin, fout, act
        for l, (lin, _) in enumerate(chains[0][:ns]):   # the trunk once, under the same offsets for every net
            for i in range(k):
                d.w_off[i][l], d.b_off[i][l] = pos, pos + lin.weight.numel()
            pos += lin.weight.numel() + lin.bias.numel()
            params += [lin.weight, lin.bias]
        for i, chain in enumerate(chains):
            for l, (lin, _) in enumerate(chain[ns:], start=ns):
                d.w_off[i][l], d.b_off[i][l] = pos, pos + lin.weight.numel()
                pos += lin.weight.numel() + lin.bias.numel()
                params += [lin.weight, lin.bias]
        if pos >= 2 ** 31:
            raise TypeError(f"{pos} parameters: cvf_mlp_desc holds 32-bit offsets")
        d.n_params = pos
        if _hip.lib().cvf_cv_nets_shared_supported(d, ns, 1) != 1:
            raise TypeError(_hip.lib().cvf_last_error().decode())
        return d, L, k, params, ns

    @staticmethod
    def _nets_plan(nets):
        """``(desc, upto_layer, k, params)`` of nets ``cvf_cv_nets_eval`` takes: the ``cvf_mlp_desc`` over the flat buffer
        ``cat(params)`` (per chain and layer: weight, bias), form A for an ``EigenFunctions`` (its nets in their own order: the
        model's outputs), form B for a bare chain.  TypeError with the reason for every other module.  Built from the modules on
        every call - nothing is kept between calls, so parameters trained or replaced in between are the ones read."""
        if type(nets) in (EigenFunctions, SharedEigenFunctions):   # (a shared trunk: its tensors once per chain in `params`)
            chains = [_strict_chain_layers(net) for net in nets.eigen_funcs]
        elif type(nets) is torch.nn.Sequential:
            chains = [_strict_chain_layers(nets)]
        else:
            raise TypeError(f"the nets are a {type(nets).__name__}: cvf_cv_nets_eval takes an EigenFunctions or a create_sequential_nn chain")
        shape = lambda c: [(lin.in_features, lin.out_features, act) for lin, act in c]
        if any(shape(c) != shape(chains[0]) for c in chains):
            raise TypeError("the nets differ in architecture")
        L = len(chains[0])
        k = len(chains) if len(chains) > 1 else chains[0][-1][0].out_features
        if not 1 <= len(chains) <= _hip.MAX_NETS:
            raise TypeError(f"k = {len(chains)} nets: the kernels take 1 to {_hip.MAX_NETS}")
        if L > _hip.MAX_LAYERS:
            raise TypeError(f"{L} layers: the kernels take 1 to {_hip.MAX_LAYERS}")
        d, params, pos = _hip.MLPDesc(), [], 0
        d.n_nets, d.n_layers = len(chains), L
        for l, (fin, fout, act) in enumerate(shape(chains[0])):
            d.dims[l], d.dims[l + 1], d.act[l] = fin, fout, act
        for i, chain in enumerate(chains):
            for l, (lin, _) in enumerate(chain):
                d.w_off[i][l], d.b_off[i][l] = pos, pos + lin.weight.numel()
                pos += lin.weight.numel() + lin.bias.numel()
                params += [lin.weight, lin.bias]
        if pos >= 2 ** 31:
            raise TypeError(f"{pos} parameters: cvf_mlp_desc holds 32-bit offsets")
        d.n_params = pos
        if _hip.lib().cvf_cv_nets_supported(d, L, 1) != 1:
            raise TypeError(_hip.lib().cvf_last_error().decode())
        return d, L, k, params

    def _derivatives(self, X, chunk, want_m, a=None):
        X = self._frames_in(X)
        dev = _hip.require_gpu(self._compute_device())
        src_dev, src_dt = X.device, (X.dtype if X.dtype.is_floating_point else torch.float32)
        B, frame_shape = int(X.shape[0]), tuple(X.shape[1:])
        n = int(np.prod(frame_shape))
        pp, nets = self._pp_and_nets()
        large = isinstance(pp, AlignFeatureLayer) and _hip.lib().cvf_align_feature_scratch_bytes(pp.pp_desc(), 64) > 0
        why = pp.derivative_table_limits() if large else None
        if want_m and why is not None:
            raise NotImplementedError(f"metric_tensor on MI355X: the feature list has {why} (csrc/metric_large.hip); "
                                      "jacobian() takes this layer (slow route, torch autograd through the whole map)")
        hip_route = isinstance(pp, torch.nn.Identity) or (isinstance(pp, AlignFeatureLayer) and why is None)
        plan = None
        if hip_route:
            try:
                plan = self._plan(nets)
            except TypeError:
                pass    # (nets_route() names the reason) the nets' part by torch.func
        with torch.cuda.device(dev):
            k = (plan[2] if plan is not None else self._n_cv(X[:1], dev)) if B > 0 else 0
            if hip_route and not 1 <= k <= _hip.MAX_NETS:
                raise NotImplementedError(f"jacobian / metric_tensor on MI355X: {k} CVs; the kernels take 1 to {_hip.MAX_NETS}")
            xi = torch.empty(B, k, device=dev, dtype=torch.float32)
            D = torch.empty((B, k, k) if want_m else (B, k, n), device=dev,
                            dtype=torch.float32 if hip_route else self._slow_dtype(pp))
            if B == 0:
                return xi.to(device=src_dev, dtype=src_dt), D.reshape((0, k) + ((k,) if want_m else frame_shape)).to(
                    device=src_dev, dtype=src_dt)
            a_dev = None if a is None else a.to(device=dev, dtype=torch.float32).contiguous()
            dense = None
            if hip_route and want_m and large:
                desc = pp.pp_desc()
                dense = torch.zeros(_hip.lib().cvf_metric_dense_doubles(desc), device=dev, dtype=torch.float64)
                _hip.check(_hip.lib().cvf_metric_dense_tensors(desc, _hip.ptr(a_dev), _hip.ptr(dense), _hip.stream()),
                           "cvf_metric_dense_tensors")
            c = self._chunk_frames(chunk, B, n, k, pp, dev, plan)
            theta = None
            if plan is not None:   # the nets' parameters as they are NOW, in the order of the plan's offsets
                theta = torch.cat([p_.detach().to(device=dev, dtype=torch.float32).reshape(-1) for p_ in plan[3]])
            for s0 in range(0, B, c):
                xs = X[s0:s0 + c]
                if hip_route:
                    xi[s0:s0 + xs.shape[0]], D[s0:s0 + xs.shape[0]] = self._hip_chunk(xs, pp, nets, k, want_m, a_dev, dense, dev,
                                                                                      plan, theta)
                else:
                    twin = self._autograd_twin() if isinstance(pp, AlignFeatureLayer) else self
                    xi[s0:s0 + xs.shape[0]], D[s0:s0 + xs.shape[0]] = self._slow_chunk(xs, twin, k, want_m, a, dev)
        D = D if want_m else D.reshape((B, k) + frame_shape)
        return xi.to(device=src_dev, dtype=src_dt), D.to(device=src_dev, dtype=src_dt)

    def _n_cv(self, x1, dev):
        with torch.no_grad():
            return int(self.forward(x1.to(dtype=torch.float32)).reshape(1, -1).shape[1])

    @staticmethod
    def _slow_dtype(pp):
        for t in list(pp.parameters()) + list(pp.buffers()):
            if t.is_floating_point():
                return t.dtype
        return torch.float32

    def _chunk_frames(self, chunk, B, n, k, pp, dev, plan=None):
        if chunk is not None:
            if int(chunk) < 1:
                raise ValueError(f"chunk must be a positive number of frames, got {chunk}")
            return int(chunk)
        d_r = pp.d_r if isinstance(pp, AlignFeatureLayer) else n
        if plan is not None:
            # fp32 per frame: x, features, aux, d xi / d r and q (one layout each), J rows or M, the nets' launch-to-launch images
            per = 4 * (2 * n + d_r + _hip.AUX_ROWS + 2 * k * d_r + k * n + k * k) \
                + 4 * self._nets_scratch_floats(plan, _hip.TILE) // _hip.TILE
        else:
            # fp32 per frame: x, features, aux, d xi / d r (rows, padded tiles, q), J rows or M, and torch.func's temporaries
            per = 4 * (2 * n + d_r + _hip.AUX_ROWS + 6 * k * d_r + k * n + k * k) + 64 * k * d_r
        free, _ = torch.cuda.mem_get_info(dev)
        c = int(self.JACOBIAN_MEMORY_FRACTION * free) // per // _hip.TILE * _hip.TILE
        return max(_hip.TILE, min(c, B))

    @staticmethod
    def _nets_scratch_floats(plan, B):
        """Floats of the nets' scratch for ``B`` frames: the formula of the plan's form (``plan[4]``: n_shared, 0 = forms A and B)."""
        lib = _hip.lib()
        if plan[4] > 0:
            return lib.cvf_cv_nets_shared_scratch_floats(plan[0], plan[4], B, 1)
        return lib.cvf_cv_nets_scratch_floats(plan[0], plan[1], B, 1)

    def _hip_chunk(self, xs, pp, nets, k, want_m, a_dev, dense, dev, plan=None, theta=None):
        """One chunk on the HIP route: (xi [c, k], J rows [c, k, n] or M [c, k, k]), fp32 on the device.  With a ``plan``
        (``_plan``; ``theta``: the flat parameters) the nets' part comes from ``cvf_cv_nets_eval`` (``cvf_cv_nets_shared_eval`` for a
        form-C plan), else from ``torch.func``."""
        lib, P, s = _hip.lib(), _hip.ptr, _hip.stream()
        c = int(xs.shape[0])
        x = xs.detach().to(device=dev, dtype=torch.float32).reshape(c, -1).contiguous()
        n = x.shape[1]
        T = _hip.ntiles(c)
        r = r_t = None
        if isinstance(pp, AlignFeatureLayer):
            assert n == 3 * pp.n_atoms, f"frames have {n} coordinates, the layer expects {3 * pp.n_atoms}"
            desc, d_r = pp.pp_desc(), pp.d_r
            if plan is not None:   # the nets read the tiles the alignment kernel writes
                r_t = torch.empty(T, d_r, _hip.TILE, device=dev, dtype=torch.float32)
            else:
                r = torch.empty(c, d_r, device=dev, dtype=torch.float32)
            aux = torch.empty(T, _hip.AUX_ROWS, _hip.TILE, device=dev, dtype=torch.float32)   # padded frame count
            scratch = _hip.align_scratch(desc, c, dev)
            _hip.check(lib.cvf_align_feature_fwd(desc, P(x), c, P(r_t), P(r), P(aux), P(scratch), s), "cvf_align_feature_fwd")
        else:
            desc, r, aux, scratch, d_r = identity_desc(n), x, None, None, n
        if plan is not None:
            mdesc, upto = plan[0], plan[1]
            assert mdesc.dims[0] == d_r, f"the nets take {mdesc.dims[0]} features, the preprocessing layer gives {d_r}"
            xi = torch.empty(c, k, device=dev, dtype=torch.float32)
            G = None if want_m else torch.empty(c, k, d_r, device=dev, dtype=torch.float32)
            g_t = torch.empty(T, k, d_r, _hip.TILE, device=dev, dtype=torch.float32) if want_m else None
            ws = torch.empty(self._nets_scratch_floats(plan, c), device=dev, dtype=torch.float32)
            if plan[4] > 0:   # form C: the trunk once
                _hip.check(lib.cvf_cv_nets_shared_eval(mdesc, P(theta), plan[4], P(r), P(r_t), c, P(xi), P(G), P(g_t), P(ws), s),
                           "cvf_cv_nets_shared_eval")
            else:
                _hip.check(lib.cvf_cv_nets_eval(mdesc, P(theta), upto, P(r), P(r_t), c, P(xi), P(G), P(g_t), P(ws), s), "cvf_cv_nets_eval")
            if not want_m:
                J = torch.empty(c, k, n, device=dev, dtype=torch.float32)
                _hip.check(lib.cvf_align_feature_vjp_rows(desc, P(x), c, P(aux), k, P(G), P(J), s), "cvf_align_feature_vjp_rows")
                return xi, J
            return xi, self._metric_from_tiles(desc, x, c, aux, a_dev, k, d_r, g_t, scratch, dense, dev)

        def f(v):
            y = nets(v.unsqueeze(0)).reshape(-1)
            return y, y

        G, xi = torch.func.vmap(torch.func.jacrev(f, has_aux=True))(r)   # [c, k, d_r], [c, k]
        G = G.detach().contiguous()
        if not want_m:
            J = torch.empty(c, k, n, device=dev, dtype=torch.float32)
            _hip.check(lib.cvf_align_feature_vjp_rows(desc, P(x), c, P(aux), k, P(G), P(J), s), "cvf_align_feature_vjp_rows")
            return xi.detach(), J
        g_t = torch.zeros(T * _hip.TILE, k, d_r, device=dev, dtype=torch.float32)
        g_t[:c] = G
        g_t = g_t.reshape(T, _hip.TILE, k, d_r).permute(0, 2, 3, 1).contiguous()   # [T][k][d_r][64]
        return xi.detach(), self._metric_from_tiles(desc, x, c, aux, a_dev, k, d_r, g_t, scratch, dense, dev)

    @staticmethod
    def _metric_from_tiles(desc, x, c, aux, a_dev, k, d_r, g_t, scratch, dense, dev):
        """M [c, k, k] = g_i . (J A J^T g_j) from g_t [T][k][d_r][64] (padded lanes 0): cvf_metric_apply, cvf_metric_gram."""
        lib, P, s = _hip.lib(), _hip.ptr, _hip.stream()
        q_t = torch.empty_like(g_t)
        e_t = torch.empty(g_t.shape[0], k, _hip.TILE, device=dev, dtype=torch.float32)
        _hip.check(lib.cvf_metric_apply(desc, P(x), c, P(aux), P(a_dev), k, P(g_t), P(q_t), P(e_t), P(scratch), P(dense), s),
                   "cvf_metric_apply")
        M = torch.empty(c, k, k, device=dev, dtype=torch.float32)
        _hip.check(lib.cvf_metric_gram(k, c, d_r, P(g_t), P(q_t), P(M), s), "cvf_metric_gram")
        return M

    @staticmethod
    def _slow_chunk(xs, model, k, want_m, a, dev):
        """The slow route on one chunk: torch autograd through ``model`` (the preprocessing module in its own precision, the
        nets in fp32), one backward per CV.  Frame-local maps only, as the generator loss assumes (pp.FactoredMetric)."""
        pp, nets = list(model.children())[0], list(model.children())[1:]
        dt = _CVModel._slow_dtype(pp)
        c = int(xs.shape[0])
        x = xs.detach().to(device=dev, dtype=dt).requires_grad_(True)
        with torch.enable_grad():
            y = pp(x)
            y = y.to(torch.float32)
            for m in nets:
                y = m(y)
            y = y.reshape(c, k)
            J = torch.empty(c, k, x[0].numel(), device=dev, dtype=dt)
            for i in range(k):
                g, = torch.autograd.grad(y[:, i].sum(), x, retain_graph=i + 1 < k, allow_unused=True)
                J[:, i] = 0.0 if g is None else g.reshape(c, -1)
        if not want_m:
            return y.detach(), J
        return y.detach(), torch.einsum("bin,n,bjn->bij", J, a.to(device=dev, dtype=dt), J)


class _FlatParams:
    """The model's parameters as views of one fp32 device buffer (+ gradient and Adam moments)."""

    def __init__(self, model, device):
        model.to(device=device, dtype=torch.float32)
        self.model = model
        self._views = None
        # (a shared trunk has one layout: mlp_layout() gives its layers the same offsets for every net, trunk - head 0 - head 1 ..)
        shared = isinstance(model, SharedEigenFunctions)
        if isinstance(model, EigenFunctions) and not shared and self._init_padded(model, device):
            return
        lay = mlp_layout(model)
        self.n = lay["n_params"]
        self.theta = torch.empty(self.n, device=device, dtype=torch.float32)
        self.grad = torch.zeros(self.n, device=device, dtype=torch.float32)
        pos = 0
        for p in model.parameters():
            n = p.numel()
            self.theta[pos:pos + n].copy_(p.data.reshape(-1))
            p.data = self.theta[pos:pos + n].view(p.shape)  # the module now aliases the flat buffer
            pos += n
        nets = lay["nets"]
        assert 1 <= len(nets) <= _hip.MAX_NETS, f"between 1 and {_hip.MAX_NETS} nets are supported, got {len(nets)}"
        L = len(nets[0])
        assert all(len(c) == L for c in nets) and L <= _hip.MAX_LAYERS, "nets must have the same depth (<= 12 layers)"
        d = _hip.MLPDesc()
        d.n_nets, d.n_layers, d.n_params = len(nets), L, self.n
        for l, (_, _, fin, fout, act) in enumerate(nets[0]):
            d.dims[l], d.dims[l + 1], d.act[l] = fin, fout, act
        for i, chain in enumerate(nets):
            for l, (wo, bo, fin, fout, act) in enumerate(chain):
                assert (fin, fout, act) == (d.dims[l], d.dims[l + 1], d.act[l]), "nets must share one architecture"
                d.w_off[i][l], d.b_off[i][l] = wo, bo
        self.desc = d
        # second copy of the weights as MFMA fragments (EigenFunctions nets only; see csrc/cvf_pack.hpp)
        n_pack = _hip.lib().cvf_ef_pack_floats(d) if isinstance(model, EigenFunctions) and not shared else 0
        self.packed = torch.zeros(n_pack, device=device, dtype=torch.float32) if n_pack > 0 else None
        self.repack()

    def _init_padded(self, model, device):
        """EigenFunctions whose hidden widths are NOT one of the kernels' widths (csrc/ef_mfma.hip: d0 -> H -> .. -> H -> 1 with
        H in _hip.EF_HIDDEN_WIDTHS): lay the nets out with every hidden layer padded to the next kernel width H.  The padding
        rows / columns hold zeros, and stay zero: a padded unit's pre-activation is 0, tanh(0) = 0, its outgoing weights are 0,
        so every gradient entry that touches the padding is exactly 0 and Adam / SGD leave a 0 with zero moments where it is.
        The module's parameters alias the unpadded sub-blocks (strided views), so state_dict(), load_state_dict(), forward and
        the per-CV text export see the nets the user built.  Returns False when no padding is needed or possible."""
        from .nn import _chain_layers
        chains = [_chain_layers(net) for net in model.eigen_funcs]
        L = len(chains[0])
        dims = [chains[0][0][0].in_features] + [lin.out_features for lin, _ in chains[0]]
        hidden = dims[1:-1]
        if not (2 <= L <= 6) or dims[-1] != 1 or not hidden or max(hidden) > max(_hip.EF_HIDDEN_WIDTHS):
            return False
        from .nn import ACT_TANH, ACT_RELU, ACT_ELU, ACT_LEAKY_RELU
        act0 = chains[0][0][1]
        if act0 not in (ACT_TANH, ACT_RELU, ACT_ELU, ACT_LEAKY_RELU):   # (a padded unit must emit act(0) = 0: not Sigmoid / Softplus)
            return False
        for c in chains:
            if [c[0][0].in_features] + [lin.out_features for lin, _ in c] != dims or [a for _, a in c] != [act0] * (L - 1) + [0]:
                return False
        cand = [w for w in _hip.ef_widths(L - 1) if w >= max(hidden)]
        if not cand:                          # e.g. ONE hidden layer of 21..32 units: no kernel width to pad to - the task then
            return False                      # raises its NotImplementedError (plain layout, no fragment copy)
        H = min(cand)
        if all(h == H for h in hidden):
            return False                      # already a kernel shape: plain layout
        pdims = [dims[0]] + [H] * (L - 1) + [1]
        per_net = sum(pdims[l + 1] * pdims[l] + pdims[l + 1] for l in range(L))
        assert len(chains) <= _hip.MAX_NETS, f"between 1 and {_hip.MAX_NETS} nets are supported, got {len(chains)}"
        self.n = per_net * len(chains)
        self.theta = torch.zeros(self.n, device=device, dtype=torch.float32)
        self.grad = torch.zeros(self.n, device=device, dtype=torch.float32)
        d = _hip.MLPDesc()
        d.n_nets, d.n_layers, d.n_params = len(chains), L, self.n
        for l in range(L):
            d.dims[l], d.dims[l + 1], d.act[l] = pdims[l], pdims[l + 1], (act0 if l < L - 1 else 0)
        self._views, pos = [], 0
        for i, chain in enumerate(chains):
            for l, (lin, _) in enumerate(chain):
                fo, fi = pdims[l + 1], pdims[l]
                d.w_off[i][l], d.b_off[i][l] = pos, pos + fo * fi
                for prm, off, shape in ((lin.weight, pos, (fo, fi)), (lin.bias, pos + fo * fi, (fo,))):
                    sl = tuple(slice(0, n_) for n_ in prm.shape)
                    tv = self.theta[off:off + int(np.prod(shape))].view(shape)[sl]
                    gv = self.grad[off:off + int(np.prod(shape))].view(shape)[sl]
                    tv.copy_(prm.data)
                    prm.data = tv                       # the module aliases its sub-block of the padded layer
                    self._views.append((prm, gv))
                pos += fo * fi + fo
        # (grad_views() must follow model.parameters() order for the optimizer's param_groups; both walk nets, then layers)
        assert [id(p_) for p_, _ in self._views] == [id(p_) for p_ in model.parameters()]
        self.desc = d
        n_pack = _hip.lib().cvf_ef_pack_floats(d)
        self.packed = torch.zeros(n_pack, device=device, dtype=torch.float32) if n_pack > 0 else None
        self.repack()
        return True

    def grad_views(self):
        """[(module parameter, its slice of the flat gradient)] in flat order."""
        if self._views is not None:
            return list(self._views)
        out, pos = [], 0
        for p in self.model.parameters():
            out.append((p, self.grad[pos:pos + p.numel()].view(p.shape)))
            pos += p.numel()
        return out

    def repack(self):
        """Rebuild the fragment copy from theta (needed after the parameters were written from outside)."""
        if self.packed is not None:
            _hip.check(_hip.lib().cvf_ef_pack(self.desc, _hip.ptr(self.theta), _hip.ptr(self.packed), _hip.stream()),
                       "cvf_ef_pack")


class _SharedTrunkFlat:
    """Flat buffer of k scalar nets whose first ``n_shared`` Linear layers are ONE set of parameters (csrc/ef_general.hip:
    cvf_ef_general_shared_*): the trunk's layers once, then net by net the layers from ``n_shared`` on.  No module aliases it - the
    owner writes ``theta`` and reads ``grad`` (RegAutoEncoderTask's generator-mode regulariser: :class:`_RegGenerator`)."""

    def __init__(self, dims, acts, k, n_shared, device):
        L = len(dims) - 1
        d = _hip.MLPDesc()
        d.n_nets, d.n_layers = k, L
        for l in range(L):
            d.dims[l], d.dims[l + 1], d.act[l] = dims[l], dims[l + 1], int(acts[l])
        pos = 0
        for l in range(n_shared):
            for i in range(k):
                d.w_off[i][l], d.b_off[i][l] = pos, pos + dims[l + 1] * dims[l]
            pos += dims[l + 1] * (dims[l] + 1)
        for i in range(k):
            for l in range(n_shared, L):
                d.w_off[i][l], d.b_off[i][l] = pos, pos + dims[l + 1] * dims[l]
                pos += dims[l + 1] * (dims[l] + 1)
        d.n_params = pos
        self.desc, self.n, self.n_shared, self.packed = d, pos, n_shared, None
        self.theta = torch.zeros(pos, device=device, dtype=torch.float32)
        self.grad = torch.zeros(pos, device=device, dtype=torch.float32)

    def grad_views(self):
        return []

    def repack(self):
        pass


class _FusedOptimizer:
    """``optimizer`` attribute of the tasks: Adam / SGD as ONE kernel over the flat buffer (same update rule and
    defaults as the ``torch.optim`` objects built at core.py:163-166), with the parts of the ``torch.optim.Optimizer``
    surface user code touches: ``param_groups`` (``param_groups[0]['lr']`` may be edited between steps - a manual decay, or a
    schedule driven by user code; ``torch.optim.lr_scheduler`` classes insist on a ``torch.optim.Optimizer`` and do not take this
    object - and is honoured by captured hipGraphs too: the kernels read it from a device scalar), ``zero_grad``, ``step``,
    ``state_dict`` / ``load_state_dict`` (the reference never checkpoints the optimizer; SURVEY 8f row 2 asks for it)."""

    def __init__(self, flat, name, lr):
        self.flat, self.name, self.lr = flat, name.lower(), float(lr)
        self.betas, self.eps = (0.9, 0.999), 1e-8
        self.exp_avg = torch.zeros_like(flat.theta)
        self.exp_avg_sq = torch.zeros_like(flat.theta)
        self.step_count = torch.zeros(1, device=flat.theta.device, dtype=torch.int32)
        self.param_groups = [dict(params=[p for p, _ in flat.grad_views()], lr=self.lr, betas=self.betas, eps=self.eps,
                                  weight_decay=0, amsgrad=False)]
        self.lr_dev = torch.full((1,), self.lr, device=flat.theta.device, dtype=torch.float32)
        self._lr_written = self.lr

    def sync_lr(self):
        """Write ``param_groups[0]['lr']`` to the device scalar the kernels read, if it changed since the last write
        (called before every eager step and before every graph replay)."""
        lr = float(self.param_groups[0]["lr"])
        if lr != self._lr_written:
            self.lr_dev.fill_(lr)
            self._lr_written = lr
        return lr

    def zero_grad(self, set_to_none=True):
        # the backward kernels overwrite the whole flat gradient; module-level .grad tensors (copies made by the
        # tasks' backward()) are dropped or zeroed as torch.optim does
        for p, _ in self.flat.grad_views():
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.zero_()

    def fused_args(self):
        """``cvf_adam_args`` for the kernels that reduce the gradient and apply Adam in one launch
        (single-process runs only: with several ranks the gradient all-reduce sits in between)."""
        if self.name != "adam":
            return None
        f, a = self.flat, _hip.AdamArgs()
        a.theta, a.m, a.v = f.theta.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr()
        a.lr, a.beta1, a.beta2, a.eps = self.sync_lr(), self.betas[0], self.betas[1], self.eps
        a.lr_dev = self.lr_dev.data_ptr()
        a.step_count = self.step_count.data_ptr()
        if f.packed is not None:
            a.mlp, a.packed = C_pointer(f.desc), f.packed.data_ptr()
        return a

    def step(self, advance=True):
        """``advance=False`` when the gradient kernel of this step has already advanced the step counter
        (the fused training loops); the public ``loss -> backward() -> optimizer.step()`` path advances here and
        takes the gradient from the modules' ``.grad`` tensors where they are set (so that edits made after
        ``backward()`` - clipping, masking - count, as with ``torch.optim``)."""
        f, lib = self.flat, _hip.lib()
        lr = self.sync_lr()
        if advance:
            self.step_count += 1
            for p, gv in f.grad_views():
                if p.grad is not None:
                    gv.copy_(p.grad.to(device=gv.device, dtype=gv.dtype))
        if self.name == "adam":
            _hip.check(lib.cvf_adam_step(_hip.ptr(f.theta), _hip.ptr(f.grad), _hip.ptr(self.exp_avg), _hip.ptr(self.exp_avg_sq),
                                         f.n, lr, _hip.ptr(self.lr_dev), self.betas[0], self.betas[1], self.eps,
                                         _hip.ptr(self.step_count), f.desc, _hip.ptr(f.packed), _hip.stream()), "cvf_adam_step")
        else:
            _hip.check(lib.cvf_sgd_step(_hip.ptr(f.theta), _hip.ptr(f.grad), f.n, lr, _hip.ptr(self.lr_dev), f.desc,
                                        _hip.ptr(f.packed), _hip.stream()), "cvf_sgd_step")

    def state_dict(self):
        """Adam moments, step number and hyper-parameters as CPU tensors / numbers (flat order = ``parameters()`` order for
        EigenFunctions / AutoEncoder models, the chain order of ``_RegFlatParams`` for RegAutoEncoder)."""
        return dict(name=self.name, n=int(self.flat.n), step=int(self.step_count.item()),
                    exp_avg=self.exp_avg.detach().cpu().clone(), exp_avg_sq=self.exp_avg_sq.detach().cpu().clone(),
                    param_groups=[dict(lr=float(self.param_groups[0]["lr"]), betas=tuple(self.betas), eps=float(self.eps))])

    def load_state_dict(self, sd):
        assert sd["name"] == self.name and int(sd["n"]) == int(self.flat.n), \
            f"optimizer state is for {sd['name']} over {sd['n']} parameters, this one is {self.name} over {self.flat.n}"
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.step_count.fill_(int(sd["step"]))
        self.param_groups[0]["lr"] = float(sd["param_groups"][0]["lr"])
        self.sync_lr()


class TrainingTask(ABC):
    """Base class of the training tasks (constructor arguments and attributes as core.py:102-143)."""

    def __init__(self, traj_obj, pp_layer, model, model_path, learning_rate, load_model_filename, save_model_every_step,
                 k, batch_size, num_epochs, test_ratio, optimizer_name, device, plot_class, plot_frequency, verbose,
                 debug_mode):
        self.device = _hip.require_gpu(device)
        self.traj_obj = traj_obj
        self.preprocessing_layer = pp_layer.to(self.device)
        self.learning_rate = learning_rate
        self.batch_size = batch_size
        self.num_epochs = num_epochs
        self.test_ratio = test_ratio
        self.k = k
        self.model = model
        self.load_model_filename = load_model_filename
        self.save_model_every_step = save_model_every_step
        self.model_path = model_path
        self.optimizer_name = optimizer_name
        self.plot_class = plot_class
        self.plot_frequency = plot_frequency
        self.verbose = verbose
        self.debug_mode = debug_mode
        self.model_name = type(self).__name__
        if self.verbose:
            print('\n[Info] Log directory: {}\n'.format(self.model_path), flush=True)
        self.writer = _SummaryWriter(self.model_path) if _SummaryWriter is not None else _ScalarLog(self.model_path)

    # -- every kernel launch goes through here; bench.py sets ``_events`` to time launches with HIP events
    _events = None
    _last_call = None      # with ``_events``: name -> (fn, args) of the most recent launch (bench.py re-times the dominant one)

    def _call(self, name, fn, *args):
        ev = self._events
        if ev is not None:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            rc = fn(*args)
            b.record()
            ev.setdefault(name, []).append((a, b))
            if self._last_call is not None:
                self._last_call[name] = (fn, args)
        else:
            rc = fn(*args)
        _hip.check(rc, name)

    def _allreduce(self, name, t):
        """One of the step's two cross-rank sums, bracketed by HIP events like a C-ABI call when the
        per-call timing pass is on (bench.py reports them per collective: where a multi-GPU step's time goes)."""
        ev = self._events
        if ev is not None and _dist.collectives() and t.is_cuda:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _dist.allreduce_sum_(t)
            b.record()
            ev.setdefault(name, []).append((a, b))
        else:
            _dist.allreduce_sum_(t)
        return t

    # -- description of r(x) for the kernels
    def _pp_desc(self, n_coord):
        pp = self.preprocessing_layer
        if isinstance(pp, torch.nn.Identity):
            return identity_desc(n_coord)
        if isinstance(pp, AlignFeatureLayer):
            assert n_coord == 3 * pp.n_atoms, f"trajectory frames have {n_coord} coordinates, layer expects {3 * pp.n_atoms}"
            return pp.pp_desc()
        raise TypeError("pp_layer must be torch.nn.Identity or a colvarsfinder.pp.AlignFeatureLayer "
                        f"(PreprocessingANN); the GPU kernels cannot run an arbitrary module ({type(pp).__name__})")

    def _load_model(self):
        """core.py:156-161: optional restart from ``load_model_filename``."""
        if self.load_model_filename:
            if os.path.isfile(self.load_model_filename):
                self.model.load_state_dict(torch.load(self.load_model_filename, map_location="cpu"), strict=False)
                if self.verbose:
                    print(f'model parameters loaded from: {self.load_model_filename}')
            elif self.verbose:
                print(f'model file not found: {self.load_model_filename}')

    def _flat_params(self):
        """The flat HBM buffer the model's parameters alias (RegAutoEncoderTask lays out its own chain)."""
        return _FlatParams(self.model, self.device)

    def init_model_and_optimizer(self):
        """core.py:145-166: optional restart from ``load_model_filename``; Adam (case-insensitive) else SGD."""
        self._load_model()
        self._flat = self._flat_params()
        self.optimizer = _FusedOptimizer(self._flat, self.optimizer_name, self.learning_rate)

    def _dev(self, t, dtype=torch.float32):
        return None if t is None else torch.as_tensor(t).detach().to(device=self.device, dtype=dtype).contiguous()

    def backward(self):
        """Fill ``p.grad`` of the module's parameters from the flat gradient of the last step that left one."""
        for p, gv in self._flat.grad_views():
            p.grad = gv.clone()

    # -- r(x) of the two autoencoder tasks: computed once per frame, the steps read the rows
    def _probe_pp(self, frame):
        """What stands in for the kernels' description of r(x) behind a foreign module: its width ``d_r``, found on one frame."""
        with torch.no_grad():
            y = self.preprocessing_layer(torch.as_tensor(frame).to(device=self.device, dtype=torch.float32))
        return types.SimpleNamespace(d_r=int(y.reshape(1, -1).shape[1]))

    def _features(self, X):
        """Frames ``X`` (host or device) -> row-major feature rows resident in HBM: K1, or - a module this package has no kernel
        for - torch, on the device, in bounded chunks."""
        X = torch.as_tensor(X).detach()
        if self._foreign_pp:
            return module_features(self.preprocessing_layer, X, self._pp.d_r, self.device)
        X = _hip.upload_f32(X, self.device)
        n = X.shape[0]
        out = torch.empty(n, self._pp.d_r, device=self.device, dtype=torch.float32)
        if n > 0:
            _hip.check(_hip.lib().cvf_align_feature_fwd(self._pp, _hip.ptr(X), n, None, _hip.ptr(out), None,
                                                        _hip.ptr(_hip.align_scratch(self._pp, n, self.device)), _hip.stream()),
                       "cvf_align_feature_fwd")
        return out

    # -- what the three train() loops share around their steps
    def _announce(self, bs, n, n_batches):
        """The reference's opening lines (core.py:483-489), rank 0 only; every argument a (train, test) pair."""
        if _dist.rank() != 0:
            return
        print("\nTraining starts.\n%d epochs in total, batch sizes (train/test): %d/%d" % (self.num_epochs, bs[0], bs[1]))
        print("\nTrain set:\n\t%d data, %d iterations per epoch, %d iterations in total." %
              (n[0], n_batches[0], n_batches[0] * self.num_epochs), flush=True)
        print("Test set:\n\t%d data, %d iterations per epoch, %d iterations in total." %
              (n[1], n_batches[1], n_batches[1] * self.num_epochs), flush=True)

    def _epoch_logs(self, n_tr, n_te, *row):
        """Device rows the steps of an epoch write their losses to (fp64; one row where a set has no batch)."""
        return tuple(torch.zeros(max(n_, 1), *row, device=self.device, dtype=torch.float64) for n_ in (n_tr, n_te))

    def _write_epoch_means(self, names, ep, tr, te):
        """core.py:559-561, 1208-1212: the epoch's mean of every loss column to the writer (NaN where the set has no batch)."""
        mean_tr = tr.mean(0) if len(tr) else torch.full((len(names),), float("nan"))
        mean_te = te.mean(0) if len(te) else torch.full((len(names),), float("nan"))
        for i, name in enumerate(names):
            self.writer.add_scalar('%s/train' % name, mean_tr[i], ep)
            self.writer.add_scalar('%s/test' % name, mean_te[i], ep)

    def _due(self, epoch):
        """``(saving, plotting)``: whether this epoch ends a save period / a plot period (a frequency of 0: never)."""
        saving = self.save_model_every_step > 0 and epoch % self.save_model_every_step == self.save_model_every_step - 1
        plotting = self.plot_frequency > 0 and epoch % self.plot_frequency == self.plot_frequency - 1
        return saving, plotting

    def _save_latest_and_best(self, epoch, last_loss, min_loss):
        """Save "latest", and "best" where the epoch's last train loss (inf: no train batch) is a strict new minimum
        (core.py:526-528); returns the minimum so far."""
        self.save_model(epoch)
        if last_loss < min_loss:
            min_loss = last_loss
            self.save_model(epoch, 'best')
        return min_loss

    def _plot(self, epoch):
        """core.py:530-532, 720-722, 1136-1140: the CV model (and the regulariser model where the task has one) to the user's
        ``plot_class``, rank 0 only."""
        if self.plot_class is not None and _dist.rank() == 0:
            cv, reg = self.colvar_model(), self.reg_model()
            self.plot_class.plot(*((cv,) if reg is None else (cv, reg)), epoch=epoch)

    def _loss_frames(self, names):
        """core.py:563-566: ``train_loss_df`` / ``test_loss_df``, one row of column means per epoch of ``loss_list``."""
        self.train_loss_df, self.test_loss_df = (
            pd.DataFrame(torch.cat([e[i].mean(dim=0, keepdim=True) for e in self.loss_list]).numpy(), columns=names) for i in (0, 1))

    def save_model(self, epoch, description="latest"):
        """core.py:168-227: ``model.pt`` + per-CV text files (+ TorchScript CV when the layer is scriptable)."""
        _dist.check_comm()
        if _dist.rank() != 0:
            return
        if self.verbose:
            print(f"\n\nEpoch={epoch}:")
        sd = {k_: v.detach().cpu() for k_, v in self.model.state_dict().items()}
        if self.debug_mode is True:
            os.makedirs(f'{self.model_path}/models', exist_ok=True)
            torch.save(sd, f'{self.model_path}/models/model_{epoch}.pt')
        out_dir = f'{self.model_path}/{description}'
        os.makedirs(out_dir, exist_ok=True)
        torch.save(sd, f'{out_dir}/model.pt')
        for idx in range(self.k):
            for name, param in self.model.get_params_of_cv(idx):
                np.savetxt('%s/%d_' % (out_dir, idx) + name.replace('.', '_') + '.txt', param.detach().cpu().numpy())
        if self.verbose:
            print(f'  trained model saved at:\n\t{out_dir}/model.pt')
        # TorchScript export (core.py:205-226): the kernel-backed alignment layer is replaced by its pure-torch export
        # twin (export.py), so the saved files are self-contained; the GPU variant is the same module moved to the device
        from .export import scriptable_cv
        cv = scriptable_cv(self.colvar_model())
        torch.jit.script(cv).save(f'{out_dir}/scripted_cv_cpu.pt')
        torch.jit.script(copy.deepcopy(cv).to(self.device)).save(f'{out_dir}/scripted_cv_gpu.pt')
        if self.verbose:
            print(f'  script models for CVs saved at:\n\t{out_dir}/scripted_cv_cpu.pt\n\t{out_dir}/scripted_cv_gpu.pt\n', flush=True)

    @abstractmethod
    def train(self):
        pass

    @abstractmethod
    def colvar_model(self):
        pass

    @abstractmethod
    def reg_model(self):
        pass


def metric_is_isotropic(diag_coeff, n_rec):
    """True when ``diag_coeff`` (None: ones) holds ONE coefficient per record atom: ``a[3b] == a[3b+1] == a[3b+2]``, compared
    exactly in the fp32 the kernels read, for every ``b < n_rec``.  Entries past ``3 * n_rec`` belong to atoms no feature reads and
    are not compared; a NaN anywhere, or a vector shorter than ``3 * n_rec``, answers False."""
    if diag_coeff is None:
        return True
    a = torch.as_tensor(diag_coeff).detach().to(device="cpu", dtype=torch.float32).reshape(-1)
    if a.numel() < 3 * n_rec or bool(torch.isnan(a).any()):
        return False
    a = a[:3 * n_rec].reshape(n_rec, 3)
    return bool(((a[:, 0] == a[:, 1]) & (a[:, 1] == a[:, 2])).all())


class _EFRoute(NamedTuple):
    """Which launches an EigenFunctionTask step runs: decided once per task, on first use (EigenFunctionTask._route), from the
    nets, the layer and the developer switches below - every place that picks a launch reads this record.

    Switches (environment; read once, when the route is decided, except as noted):
      CVF_PIPELINE=1           align the next batch beside the backward launch (read at construction); turns the ef16 route off
      CVF_NO_EF16              generator mode: no 16-frame route (the C library reads it too, in cvf_ef16_supported)
      CVF_NO_EF16_TRANSFER     transfer mode: no 16-frame route
      CVF_EF16_ISO=0           generator mode, 16-frame route: the general (laboratory-frame) passes of q = J A J^T g even where
                               diag_coeff is isotropic (read at construction: EigenFunctionTask.metric_isotropic)
      CVF_NO_TRANSFER_ROWS     ef16 transfer mode: the front launch without unit rows + cvf_ef_stats
      CVF_NO_ALIGN_FWD         transfer mode: no fused alignment + forward launch (plain route instead)
      CVF_NO_FWD_METRIC        read by the C library in cvf_ef_fwd_metric_supported: no fused generator launch
      CVF_NO_ALIGN_FUSED       read by the C library in cvf_ef_align_fwd_metric_supported: alignment outside the fused launch
    """
    kind: str            # "ef16" (16 frames per wave), "fused" / "plain" (64-frame kernels) or "general" (per-layer launches)
    align_inside: bool   # the forward launch can solve the alignment itself (used when the batch is not already aligned)
    unit_rows: bool      # ef16 transfer mode: the paired front launch that leaves the units' rows of the time-lagged sums
    backward: tuple      # (call name = C function, takes packed, takes w_lag, takes q) of the backward launch
    # general route of nets that share their first `shared` layers - a SharedEigenFunctions model, or RegAutoEncoderTask's inner task:
    # cvf_ef_general_shared_* in generator mode, cvf_ef_general_shared_transfer_* in transfer mode
    shared: Optional[int] = None


class _EFWorkspace:
    """Device buffers of one batch size (all sizes follow include/cvf.h) and what the route needs to know about that size."""

    def __init__(self, B, k, d_r, n_params, lag, mlp_desc, device, route):
        lib = _hip.lib()
        ef16, general, ns = route.kind == "ef16", route.kind == "general", route.shared
        T = _hip.ntiles(B)
        Tt = 2 * T if lag > 0 else T
        f32 = dict(device=device, dtype=torch.float32)
        f64 = dict(device=device, dtype=torch.float64)
        self.B, self.T, self.Tt = B, T, Tt
        # features / alignment data are double-buffered: the alignment kernel of the NEXT batch does not depend on
        # the parameters, so the training loop runs it beside this batch's step (EigenFunctionTask.train_step)
        self.slot = 0
        self._feat = [torch.empty(Tt * d_r * _hip.TILE, **f32) for _ in range(2)]
        self._aux = [torch.empty(T * _hip.AUX_ROWS * _hip.TILE, **f32) for _ in range(2)]
        self.y = torch.empty(Tt * k * _hip.TILE, **f32)
        if lag == 0:
            self.g = None if ef16 else torch.empty(T * k * d_r * _hip.TILE, **f32)   # (the 16-frame step keeps g on the chip)
            self.q = torch.empty(T * k * d_r * _hip.TILE, **f32)
            self.e = torch.empty(T * k * _hip.TILE, **f32)
        else:
            self.g = self.q = self.e = None
        self.scratch = torch.zeros(lib.cvf_ef16_scratch_doubles(B, k) if ef16 else
                                   lib.cvf_metric_stats_scratch_doubles(B, k) if lag == 0 else
                                   lib.cvf_ef_stats_scratch_doubles(k, lag), **f64)
        self.stats = torch.empty(lib.cvf_ef_nstats(k, lag), **f64)
        self.loss_vec = torch.empty(3 + 2 * k, **f64)
        self.loss_out = self.loss_vec   # where this step's loss vector goes (_forward: the caller's row, else loss_vec)
        self.coef = torch.empty(4 * k + k * k, **f64)
        self._k1_scratch, self.k1_scratch_checked = [None, None], False   # large-molecule alignment scratch, sized on first use
        # hidden activations handed from the forward kernel to the backward kernel (0 floats: shape without hand-off)
        # (the general route, csrc/ef_general.hip: activations, the sweep of g, the tangent chain and the adjoints of every layer)
        n_saved = (lib.cvf_ef_general_shared_transfer_saved_floats(mlp_desc, Tt, ns) if ns is not None and lag > 0 else
                   lib.cvf_ef_general_shared_saved_floats(mlp_desc, Tt, ns) if ns is not None else
                   lib.cvf_ef_general_saved_floats(mlp_desc, Tt, lag) if general else
                   lib.cvf_ef16_saved_floats(mlp_desc, Tt) if ef16 else lib.cvf_ef_saved_floats(mlp_desc, Tt))
        self.saved = torch.empty(n_saved, **f32) if n_saved > 0 else None
        self.slab_rows = (lib.cvf_ef_general_shared_transfer_slab_rows(mlp_desc, Tt, ns) if ns is not None and lag > 0 else
                          lib.cvf_ef_general_shared_slab_rows(mlp_desc, Tt, ns) if ns is not None else
                          lib.cvf_ef_general_slab_rows(mlp_desc, Tt) if general else lib.cvf_ef_backward_slab_rows(Tt))
        self.slab = torch.empty(self.slab_rows * n_params, **f32)
        # the 16-frame step at this batch size: > 0 - the front launch leaves the units' rows of the batch sums in `scratch` and
        # cvf_ef16_finish[_dp] adds them; 0 - it sums them itself (generator mode) / cvf_ef_stats does (transfer mode)
        self.unit_rows = (0 if not ef16 else lib.cvf_ef16_rows(B) if lag == 0 else
                          lib.cvf_ef16_transfer_rows(B, k) if route.unit_rows else 0)
        # alignment rows and feature tile of the resident batches of this size (EigenFunctionTask._alignment_rows):
        # (X.data_ptr(), B) -> (X, X._version when they were filled, rows, tile)
        self.align_rows = {}
        self.tile = None   # the resident batch's feature tile this step's front launch read (None: it wrote `feat`)

    feat = property(lambda self: self._feat[self.slot])
    feat_in = property(lambda self: self._feat[self.slot] if self.tile is None else self.tile)   # what the backward launch reads
    aux = property(lambda self: self._aux[self.slot])
    k1_scratch = property(lambda self: self._k1_scratch[self.slot])


class _HostFrames:
    """The trajectory on the host as the tasks touch it: ``shape``, ``rows(idx)`` (the frames a process keeps resident) and
    ``all()`` (single process: everything, once).  ``traj_obj.trajectory`` may be an array (the reference's
    ``WeightedTrajectory``: held whole, core.py:343), an ``np.memmap`` (indexing it reads the pages of the rows asked for), or
    any object with ``shape`` and ``take_rows(rows)`` - ``utils.RowReader`` - so that a rank of a data-parallel job never
    holds more than its own 1/world of the frames on the host either."""

    def __init__(self, src):
        self.reader = src if hasattr(src, "take_rows") else None
        self.array = None if self.reader is not None else np.asarray(src)
        self.shape = tuple((self.reader if self.reader is not None else self.array).shape)

    def rows(self, idx):
        return self.reader.take_rows(idx) if self.reader is not None else self.array[idx]

    def all(self):
        return self.reader.take_rows(np.arange(self.shape[0])) if self.reader is not None else self.array


class EigenFunctionTask(TrainingTask):
    """Eigenfunctions of the generator (``lag_tau == 0``) or of the transfer operator (``lag_tau > 0``).

    Arguments, defaults and attributes as reference core.py:293-354 (see the module docstring for
    what replaces what).  ``loss_list`` / ``train_loss_df`` / ``test_loss_df`` hold the same
    per-step rows ``[loss, eigen_non_penalty, eigen_penalty, eig_1..k]`` as the reference.
    """

    def __init__(self, traj_obj, pp_layer, model, model_path, alpha, eig_weights, diag_coeff=None, beta=1.0, lag_tau=0,
                 learning_rate=0.01, load_model_filename=None, save_model_every_step=10, sort_eigvals_in_training=True,
                 k=1, batch_size=1000, num_epochs=10, test_ratio=0.2, optimizer_name='Adam',
                 device=torch.device('cuda'), plot_class=None, plot_frequency=0, verbose=True, debug_mode=True,
                 general_nets=False, _shared_trunk=None):
        super().__init__(traj_obj, pp_layer, model, model_path, learning_rate, load_model_filename, save_model_every_step,
                         k, batch_size, num_epochs, test_ratio, optimizer_name, device, plot_class, plot_frequency,
                         verbose, debug_mode)
        assert isinstance(model, EigenFunctions), 'model must be an object of the class EigenFunctions'
        assert k == len(model.eigen_funcs), \
            f'number of cv ({k}) must equal the number of eigenfunctions ({len(model.eigen_funcs)})'
        assert len(eig_weights) >= k, f'{k} eigenvalue weights are needed, got {len(eig_weights)}'
        self._alpha = alpha
        self._sort_eigvals_in_training = sort_eigvals_in_training
        self._eig_w = eig_weights
        self._cvec = None
        self.traj_dt = traj_obj.dt
        lag_idx = lag_tau / self.traj_dt
        assert abs(lag_idx - int(lag_idx)) < 1e-6, \
            f'lag-time ({lag_tau}) not divisable by the timestep {self.traj_dt} of the trajectory'
        self.lag_idx = int(lag_idx)
        if self.verbose:
            print('\nEigenfunctions:\n', self.model, flush=True)
        # _shared_trunk (private: RegAutoEncoderTask's inner task, _RegGenerator): dict(dims, acts, n_shared) - the k nets share
        # their first n_shared layers; `model` only states the architecture (it may live on the meta device), the parameters are
        # the owner's, in a _SharedTrunkFlat, and the step runs the shared launches of csrc/ef_general.hip
        self._n_shared = None
        if _shared_trunk is not None:
            st = _shared_trunk
            if self.lag_idx != 0:
                raise NotImplementedError("nets with a shared trunk: the private _shared_trunk option is generator-mode only; the "
                                          "transfer-mode shared step takes a nn.SharedEigenFunctions model (csrc/ef_general.hip)")
            self._flat = _SharedTrunkFlat(st["dims"], st["acts"], k, st["n_shared"], self.device)
            self.optimizer = _FusedOptimizer(self._flat, self.optimizer_name, self.learning_rate)
            if not _hip.lib().cvf_ef_general_shared_supported(self._flat.desc, st["n_shared"]):
                raise NotImplementedError(f"{_hip.lib().cvf_last_error().decode()} (csrc/ef_general.hip: cvf_ef_general_shared_supported)")
            self._n_shared = int(st["n_shared"])
        elif isinstance(model, SharedEigenFunctions):
            # a public model on a shared trunk: its parameters alias the flat buffer (trunk once, then head by head), and the step
            # runs the shared launches of csrc/ef_general.hip - generator mode the existing ones, transfer mode
            # cvf_ef_general_shared_transfer_* - whatever `general_nets` says: this model has no other route
            if _dist.world() > 1:
                raise NotImplementedError("EigenFunctionTask with a SharedEigenFunctions model runs in single-process jobs only: "
                                          "its data-parallel step (world > 1) has not been verified")
            self.init_model_and_optimizer()
            lib, ns = _hip.lib(), int(model.n_shared)
            ok = (lib.cvf_ef_general_shared_supported if self.lag_idx == 0 else lib.cvf_ef_general_shared_transfer_supported)(self._flat.desc, ns)
            if not ok:
                raise NotImplementedError(f"EigenFunctionTask with a SharedEigenFunctions model on MI355X: {lib.cvf_last_error().decode()} "
                                          "(csrc/ef_general.hip: efg_why_shared)")
            self._n_shared = ns
        else:
            self.init_model_and_optimizer()
        # general_nets: shapes without a kernel instance run the per-layer launches of csrc/ef_general.hip (shapes WITH an
        # instance, padded layouts included, keep their kernels: the option changes nothing for them)
        self._general = self._n_shared is not None
        if self._flat.packed is None and general_nets and not self._general:
            if not _hip.lib().cvf_ef_general_supported(self._flat.desc):
                raise NotImplementedError(f"EigenFunctionTask(general_nets=True) on MI355X: {_hip.lib().cvf_last_error().decode()} "
                                          "(csrc/ef_general.hip: cvf_ef_general_supported)")
            self._general = True
        if self._flat.packed is None and not self._general:   # no matrix-core kernel instance: say so here, not at the first step
            d = self._flat.desc
            raise NotImplementedError(
                "EigenFunctionTask on MI355X: no kernel instance for nets with layer widths "
                f"{[d.dims[i] for i in range(d.n_layers + 1)]}. Supported: 2 to 5 hidden layers of at most "
                f"{max(_hip.EF_HIDDEN_WIDTHS)} units each, ONE hidden layer of at most {max(_hip.ef_widths(1))} units "
                f"(kernel widths {_hip.EF_HIDDEN_WIDTHS}, for 4 or 5 hidden layers 20 and 32; "
                f"other widths are zero-padded to the next one - not with Sigmoid / Softplus, whose padding would not stay zero), "
                f"scalar output, ONE activation of include/cvf.h after every hidden layer, k <= {_hip.MAX_NETS} "
                "(csrc/ef_mfma.hip: ef_shape / ef_dispatch). Pass general_nets=True to run other shapes on the per-layer "
                "kernels of csrc/ef_general.hip.")

        # The frames stay resident in HBM (core.py:343-344 keeps CPU copies and moves every batch, core.py:500).  One process:
        # the whole trajectory.  Data-parallel job (one process per GPU): NOT here - train() uploads only the rows of this
        # rank's slices of the static batches, 1/world of the trajectory per GPU.
        self._traj_host = _HostFrames(traj_obj.trajectory)
        self._n_frames = int(self._traj_host.shape[0])
        self._sharded = _dist.world() > 1
        self.tot_dim = int(np.prod(self._traj_host.shape[1:]))
        self._beta = beta
        if self.lag_idx == 0:
            if diag_coeff is not None:
                assert diag_coeff.dim() == 1 and diag_coeff.size(dim=0) == self.tot_dim, \
                    f'diag_coeff should be a 1d tensor of length {self.tot_dim}, current shape: {diag_coeff}'
                self._diag_coeff = diag_coeff.detach().to(device=self.device, dtype=torch.float32).contiguous()
            else:
                self._diag_coeff = torch.ones(self.tot_dim, device=self.device, dtype=torch.float32)
        # pp_layer may be ANY torch module (core.py:65,122,403): `_frames` maps the trajectory's frames to what the kernels take -
        # the frames themselves (Identity, AlignFeatureLayer), the feature rows r(x) (transfer operator: run on identity_desc) or,
        # in generator mode, one record [r(x) | L] per frame with L L^T = J A J^T (pp.FactoredMetric, CVF_PP_FACTORED)
        self._foreign_pp = not isinstance(self.preprocessing_layer, (torch.nn.Identity, AlignFeatureLayer))
        self._fm = None
        if self._foreign_pp:
            if self._sharded:
                raise NotImplementedError("EigenFunctionTask with a preprocessing module other than Identity / AlignFeatureLayer "
                                          "runs in single-process jobs only (the per-rank record building is not there)")
            probe = self._traj_host.rows(np.arange(min(2, self._n_frames)))
            if self.lag_idx == 0:
                self._fm = FactoredMetric(self.preprocessing_layer, self._traj_host.shape[1:], self._diag_coeff, self.device, probe)
                self._pp = self._fm.desc()
                self._check_record_memory(self._fm.record_bytes(self._n_frames))
            else:
                with torch.no_grad():
                    y = self.preprocessing_layer(torch.as_tensor(np.asarray(probe)).to(device=self.device, dtype=torch.float32))
                self._pp = identity_desc(int(y.reshape(y.shape[0], -1).shape[1]))
        else:
            self._pp = self._pp_desc(self.tot_dim)
        # One coefficient per record atom (ones, 1 / mass): the 16-frame front launch forms q = J A J^T g in the aligned frame
        # (`cfg.iso_metric`, include/cvf.h).  Decided once, here; CVF_EF16_ISO=0 keeps the general passes.
        self.metric_isotropic = (self.lag_idx == 0 and not self._foreign_pp and os.environ.get("CVF_EF16_ISO", "1") != "0"
                                 and metric_is_isotropic(diag_coeff, int(self._pp.n_rec)))
        self._traj = None if self._sharded else self._frames(self._traj_host.all())
        self._weights = torch.as_tensor(np.asarray(traj_obj.weights)).to(device=self.device, dtype=torch.float32).contiguous()
        self.resident_bytes = 0 if self._sharded else self._traj.numel() * 4    # frames (or records) held in HBM (train() adds its gathers)
        assert self._pp.d_r == self._flat.desc.dims[0], \
            f'preprocessing layer emits {self._pp.d_r} features but the networks take {self._flat.desc.dims[0]}'
        cfg = _hip.EFCfg()
        cfg.k, cfg.lag_idx, cfg.sort_eigvals = k, self.lag_idx, int(bool(sort_eigvals_in_training))
        cfg.iso_metric = int(self.metric_isotropic)
        cfg.alpha, cfg.beta, cfg.dt = float(alpha), float(beta), float(self.traj_dt)
        for i in range(k):
            cfg.eig_w[i] = float(eig_weights[i])
        self._cfg = cfg
        # large molecules (streaming alignment path): moments of (diag_coeff, reference) used by the derivative kernel
        self._dense = None
        if self.lag_idx == 0 and _hip.lib().cvf_align_feature_scratch_bytes(self._pp, 64) > 0:
            why = self.preprocessing_layer.derivative_table_limits()
            if why is not None:   # (here, not as a generic message at the first step)
                raise NotImplementedError(f"EigenFunctionTask (generator mode) on MI355X: the feature list has {why} "
                                          "(csrc/metric_large.hip). Use lag_tau > 0 (no derivative through the features) or fewer features per atom.")
            self._dense = torch.zeros(_hip.lib().cvf_metric_dense_doubles(self._pp), device=self.device, dtype=torch.float64)
            _hip.check(_hip.lib().cvf_metric_dense_tensors(self._pp, _hip.ptr(self._diag_coeff), _hip.ptr(self._dense),
                                                           _hip.stream()), "cvf_metric_dense_tensors")
        if self.lag_idx == 0 and self._pp.mode == _hip.PP_FEATURES:   # a layer without alignment: the limits of csrc/k1_features.hip
            why = self.preprocessing_layer.derivative_table_limits()
            if why is not None:
                raise NotImplementedError(f"EigenFunctionTask (generator mode) on MI355X: the feature list has {why} "
                                          "(csrc/k1_features.hip). Use lag_tau > 0 (no derivative through the features) or fewer features.")
        self._ws = {}
        self._graphs = {}
        # whole-step hipGraph replay (CVF_GRAPH=0 turns it off).  In a data-parallel job the two RCCL all-reduces are
        # captured inside the graph (backend nccl only; a failed capture falls back to eager launches for good)
        self._use_graphs = os.environ.get("CVF_GRAPH", "1") != "0" and (not _dist.collectives() or _dist.backend() == "nccl" or
                                                                        _dist.fused_comm() is not None)   # (the peer-to-peer kernels capture on any backend)
        self._route_record = None   # which launches a step runs (`_route`): decided on first use
        # (RegAutoEncoderTask drives an inner task of this class: `_local_only` - evaluate the batch handed in on this rank alone, no
        #  cross-rank sums; `_grad_local` - leave the parameter gradient un-reduced, the caller sums its own flat gradient later)
        self._local_only = self._grad_local = False
        self._side = torch.cuda.Stream(device=self.device)
        # CVF_PIPELINE=1: the next batch's alignment (independent of the parameters) runs on this stream beside the
        # current step's backward kernel.  Off by default: at 20 000 frames per step it measured 133 us/step against
        # 126 serial - the two-branch graph costs more at the fork/join than the 14 us kernel it hides.
        self._pipeline = os.environ.get("CVF_PIPELINE", "0") == "1"
        # CVF_ALIGN_CACHE=0: every train step solves its frames' alignment again (see _alignment_rows); read once, here
        self._align_cache = os.environ.get("CVF_ALIGN_CACHE", "1") != "0"
        self.alignment_fills = 0   # launches of cvf_ef16_align_rows_tile so far (one per resident batch and per re-fill)

    # ---------------------------------------------------------------- model views
    def get_reordered_eigenfunctions(self, model, cvec):
        """core.py:356-370: deep copy whose module list is re-ordered by ``cvec``."""
        new = copy.deepcopy(model)
        if isinstance(model, SharedEigenFunctions):   # the copy's own chains re-ordered: they keep sharing the copy's trunk
            new.eigen_funcs = torch.nn.ModuleList([new.eigen_funcs[int(i)] for i in cvec])
            return new
        new.eigen_funcs = torch.nn.ModuleList([copy.deepcopy(model.eigen_funcs[int(i)]) for i in cvec])
        return new

    def colvar_model(self):
        """core.py:372-382: ``Sequential(preprocessing_layer, nets re-ordered by the last cvec)``."""
        if self._cvec is None:
            self._cvec = torch.arange(self.k)
        return _CVModel(self.preprocessing_layer, self.get_reordered_eigenfunctions(self.model, self._cvec), device=self.device)

    def reg_model(self):
        return None

    # share of the free device memory the resident records and train()'s gathered copy of them may take
    RECORD_MEMORY_FRACTION = 0.8

    def _check_record_memory(self, nbytes):
        """Records of every frame stay resident and train() gathers one epoch's copy of them: both must fit."""
        free, _ = torch.cuda.mem_get_info(self.device)
        need = 2 * int(nbytes)
        if need > self.RECORD_MEMORY_FRACTION * free:
            raise NotImplementedError(
                f"EigenFunctionTask (generator mode) with a {type(self.preprocessing_layer).__name__} preprocessing module: the "
                f"per-frame records take {int(nbytes)} bytes, {need} with train()'s gathered copy, more than "
                f"{self.RECORD_MEMORY_FRACTION:.0%} of the {int(free)} bytes free on the device. Use lag_tau > 0 (features only) or "
                "fewer features.")

    def _frames(self, X):
        """What the kernels take for the frames ``X`` (host or device, ``[B, *frame_shape]``): the frames themselves, or - with a
        foreign preprocessing module - records (generator mode) or feature rows (transfer operator), on the device."""
        if not self._foreign_pp:
            return _hip.upload_f32(X, self.device)
        if self._fm is not None:
            return self._fm.records(X)
        return module_features(self.preprocessing_layer, X, self._pp.d_r, self.device)

    # ---------------------------------------------------------------- GPU step
    def _workspace(self, B):
        ws = self._ws.get(B)
        if ws is None:
            ws = self._ws[B] = _EFWorkspace(B, self.k, self._pp.d_r, self._flat.n, self.lag_idx, self._flat.desc, self.device,
                                            self._route)
        return ws

    @property
    def _route(self):
        """The step's launches (:class:`_EFRoute`), decided on first use: the ONE place that reads the route's switches."""
        if self._route_record is None:
            lib, fl, pp, env, gen = _hip.lib(), self._flat, self._pp, os.environ, self.lag_idx == 0
            if self._general:      # (no kernel instance: none of the queries below would say yes)
                r = _EFRoute("general", False, False, ("cvf_ef_general_backward", False, True, True), self._n_shared)
            elif (not self._pipeline and env.get("CVF_NO_EF16" if gen else "CVF_NO_EF16_TRANSFER") is None
                    and bool(lib.cvf_ef16_supported(fl.desc, pp))):
                r = _EFRoute("ef16", True, not gen and env.get("CVF_NO_TRANSFER_ROWS") is None,
                             ("cvf_ef16_backward", True, False, True) if gen else ("cvf_ef16_backward_transfer", True, True, False))
            else:
                if gen:   # [alignment,] nets forward, q = J A J^T g, E and the batch sums in one launch: g never leaves the chip
                    fused = bool(lib.cvf_ef_fwd_metric_supported(fl.desc, pp))
                    inside = fused and bool(lib.cvf_ef_align_fwd_metric_supported(fl.desc, pp))
                else:     # alignment + forward of both frame sets in one launch
                    fused = inside = env.get("CVF_NO_ALIGN_FWD") is None and bool(lib.cvf_ef_align_fwd_metric_supported(fl.desc, pp))
                r = _EFRoute("fused" if fused else "plain", inside, False, ("cvf_ef_backward", True, True, True))
            self._route_record = r
        return self._route_record

    def _use_ef16(self):
        """The fast layout: the 16-frames-per-wave step (csrc/ef16_front.hip, ef16_back.hip; generator and transfer-operator mode)."""
        return self._route.kind == "ef16"

    def _alignment_rows(self, ws, X):
        """``(rows, tile)`` of the resident batch ``X`` - its alignment rows (csrc/ef16_front_rows.hip: rotation, centroid and
        K^-1 of every frame, 84 bytes per frame) and its feature tile (the aligned positions as the backward launch reads them,
        ``Tt * d_r * 64`` floats: 264 bytes per frame at d_r = 66) - filled by one launch on its first visit, or None: this step's
        front launch derives both itself.

        Both depend on the frames and the layer only, and the training loops replay the same static batches every epoch
        (shuffle=False, core.py:472-481), so every visit after the first starts from them.  An entry is keyed by the batch's
        address and size and HOLDS ``X``: its memory cannot be handed to another tensor while the entry lives, and an in-place
        torch write to ``X`` or its base changes ``X._version`` and re-fills.  A write torch cannot see (a raw kernel, another
        library) is the caller's to announce with :meth:`drop_alignment_cache`.  Entries are never evicted (a captured graph may
        hold the pointers) and are created - rows and tile together or not at all - only while all of them together stay within
        the share of the free device memory that RECORD_MEMORY_FRACTION leaves over; nothing is allocated while the stream is
        capturing."""
        if not self._align_cache:
            return None
        key = (X.data_ptr(), ws.B)
        ent = ws.align_rows.get(key)
        if ent is not None and ent[1] == X._version:
            return ent[2], ent[3]
        if torch.cuda.is_current_stream_capturing():
            return None
        lib = _hip.lib()
        if ent is None:
            n_rows, n_tile = int(lib.cvf_ef16_align_rows_floats(ws.B)), ws.Tt * self._pp.d_r * _hip.TILE
            free, _ = torch.cuda.mem_get_info(self.device)
            if self.alignment_rows_bytes + self.feature_tile_bytes + 4 * (n_rows + n_tile) > (1.0 - self.RECORD_MEMORY_FRACTION) * free:
                return None
            rows = torch.empty(n_rows, device=self.device, dtype=torch.float32)
            tile = torch.empty(n_tile, device=self.device, dtype=torch.float32)
        else:
            rows, tile = ent[2], ent[3]   # (the same buffers: a captured graph may hold their addresses)
        # (not through _call: its event log holds the launches of a STEP - bench.py's launches_per_step, the launch checks of the
        #  tests; this one happens once per resident batch and is counted in `alignment_fills`)
        _hip.check(lib.cvf_ef16_align_rows_tile(self._pp, _hip.ptr(X), ws.B, _hip.ptr(rows), _hip.ptr(tile), _hip.stream()),
                   "cvf_ef16_align_rows_tile")
        self.alignment_fills += 1
        ws.align_rows[key] = (X, X._version, rows, tile)
        return rows, tile

    @property
    def alignment_rows_bytes(self):
        """Device memory the alignment rows of the resident batches take now (84 bytes per frame; beside ``resident_bytes``, which
        counts the frames themselves)."""
        return sum(e[2].numel() * 4 for ws in self._ws.values() for e in ws.align_rows.values())

    @property
    def feature_tile_bytes(self):
        """Device memory the feature tiles of the resident batches take now (``4 * Tt * d_r * 64`` bytes each: 264 bytes per
        frame at d_r = 66), beside ``alignment_rows_bytes``."""
        return sum(e[3].numel() * 4 for ws in self._ws.values() for e in ws.align_rows.values())

    def drop_alignment_cache(self):
        """Forget the alignment rows and the feature tile of every resident batch, and the captured graphs that read them.  Call
        it after writing to a batch's frames by means torch does not see; ``task._ws.clear()`` releases them too (with the
        workspaces)."""
        self._graphs.clear()
        for ws in self._ws.values():
            ws.align_rows.clear()

    def _sum_stats_and_tail(self, ws):
        """Data-parallel step, collective #1 + the loss tail on this rank's batch sums in ``ws.stats``:
        one launch over the peer-to-peer windows (cvf_ef_loss_dp), else an all-reduce followed by cvf_ef_loss."""
        lib, P = _hip.lib(), _hip.ptr
        comm = _dist.fused_comm()
        if comm is not None:
            self._call("cvf_ef_loss_dp", lib.cvf_ef_loss_dp, self._cfg, P(ws.stats), P(ws.loss_out), P(ws.coef), comm, _hip.stream())
        else:
            self._allreduce("allreduce_batch_sums", ws.stats)
            self._call("cvf_ef_loss", lib.cvf_ef_loss, self._cfg, P(ws.stats), P(ws.loss_out), P(ws.coef), _hip.stream())

    def _align(self, ws, slot, X, X_lag):
        """K1 of one batch (and of its lagged partner) into feature buffer ``slot``."""
        lib, P = _hip.lib(), _hip.ptr
        B, d_r = ws.B, self._pp.d_r
        self._call("cvf_align_feature_fwd", lib.cvf_align_feature_fwd, self._pp, P(X), B, P(ws._feat[slot]), None, P(ws._aux[slot]),
                   P(ws._k1_scratch[slot]), _hip.stream())
        if self.lag_idx > 0:
            feat_lag = ws._feat[slot][ws.T * d_r * _hip.TILE:]
            self._call("cvf_align_feature_fwd", lib.cvf_align_feature_fwd, self._pp, P(X_lag), B, P(feat_lag), None, None,
                       P(ws._k1_scratch[slot]), _hip.stream())

    def _forward(self, X, w, X_lag=None, w_lag=None, slot=0, aligned=False, out=None, cache=False):
        """Everything up to the loss for one (local) batch; leaves loss_vec / coef on the device.
        ``aligned``: buffer ``slot`` already holds this batch's features (a previous step prefetched them).
        ``cache``: ``X`` is a resident batch that will be visited again (the training loops): generator mode on the 16-frame
        route keeps its alignment rows (:meth:`_alignment_rows`) - same results bit for bit.
        ``out``: fp64 device row of length 3 + 2k that receives the loss vector instead of ``ws.loss_vec`` (the training
        loops pass the step's slot of the epoch log: no copy kernel per step)."""
        route, s, P = self._route, _hip.stream(), _hip.ptr
        assert not (aligned and route.kind == "ef16"), \
            "the 16-frame step aligns inside its front launch: there is no prefetched feature buffer to start from (CVF_PIPELINE=1 turns it off)"
        ws = self._workspace(X.shape[0])
        ws.slot, ws.tile = slot, None
        single = not _dist.collectives() or self._local_only   # no cross-rank reduction: the loss tail runs inside the stats launch
        ws.loss_out = ws.loss_vec if out is None else out
        assert ws.loss_out.is_contiguous() and ws.loss_out.dtype == torch.float64 and ws.loss_out.numel() == 3 + 2 * self.k
        lv, cf = (P(ws.loss_out), P(ws.coef)) if single else (None, None)
        if route.kind != "ef16" and not ws.k1_scratch_checked:
            ws._k1_scratch = [_hip.align_scratch(self._pp, ws.B, self.device) for _ in range(2)]
            ws.k1_scratch_checked = True
        fwd = ((self._fwd_ef16_gen if self.lag_idx == 0 else self._fwd_ef16_tr) if route.kind == "ef16" else
               self._fwd_fused_gen if route.kind == "fused" and self.lag_idx == 0 else self._fwd_separate)
        # The route's launches.  `fin`: the launch that finishes the batch sums, left to the rule below - (call name, C function,
        # its `_dp` twin or None, arguments up to `stats`) - or None: the forward launch took `stats` (and `lv`, `cf`) itself.
        fin = fwd(ws, X, w, X_lag, w_lag, aligned, cache, lv, cf)
        # Who adds the rows, who sums over the ranks, who runs the loss tail:
        if fin is not None:
            name, fn, fn_dp, head = fin
            comm = None if single or fn_dp is None else _dist.fused_comm()
            if comm is not None:   # 2. rows -> sums -> collective #1 -> loss tail in ONE launch over the peer-to-peer windows
                self._call(fn_dp.__name__, fn_dp, *head, P(ws.stats), P(ws.loss_out), P(ws.coef), comm, s)
                return ws
            self._call(name, fn, *head, P(ws.stats), lv, cf, s)   # 1. (single: `lv`, `cf` set) it runs the loss tail itself
        if not single:                                            # 3. else collective #1 and the tail follow the sums
            self._sum_stats_and_tail(ws)
        return ws

    def _fwd_ef16_gen(self, ws, X, w, X_lag, w_lag, aligned, cache, lv, cf):
        """coordinates -> features, y, hidden activations, q = J A J^T g, E and the batch sums in one launch, 16 frames per wave;
        the units' rows of the sums are left to cvf_ef16_finish[_dp] (batches past cvf_ef16_rows: summed in the front launch)."""
        lib, fl, s, P = _hip.lib(), self._flat, _hip.stream(), _hip.ptr
        al = self._alignment_rows(ws, X) if cache else None
        if al is not None:
            ws.tile = al[1]   # the front launch reads the batch's tile, and so does the backward launch (`ws.feat_in`)
        args = (fl.desc, P(fl.theta), P(fl.packed), P(ws.feat_in), self._pp, P(X), ws.B, P(self._diag_coeff), P(ws.y), P(ws.saved),
                P(ws.q), P(ws.e), self._cfg, P(w), P(ws.scratch), None if ws.unit_rows else P(ws.stats), lv, cf)
        # (an isotropic metric travels in `self._cfg.iso_metric`: the same two entry points, their aligned-frame passes)
        if al is not None:   # (the same name for either form: one call of the step, the same outputs)
            self._call("cvf_ef16_front", lib.cvf_ef16_front_rows, *args, P(al[0]), s)
        else:
            self._call("cvf_ef16_front", lib.cvf_ef16_front, *args, s)
        if ws.unit_rows:
            return "cvf_ef16_finish", lib.cvf_ef16_finish, lib.cvf_ef16_finish_dp, (self._cfg, ws.B, P(ws.scratch))
        return None

    def _fwd_ef16_tr(self, ws, X, w, X_lag, w_lag, aligned, cache, lv, cf):
        """Transfer-operator mode: coordinates of the frames and of their lagged partners -> features, y, hidden activations in one
        launch (16 frames per wave), then the time-lagged batch sums."""
        lib, fl, s, P = _hip.lib(), self._flat, _hip.stream(), _hip.ptr
        args = (fl.desc, P(fl.theta), P(fl.packed), P(ws.feat), self._pp, P(X), P(X_lag), ws.B, P(ws.y), P(ws.saved))
        if ws.unit_rows:   # a unit and its lagged partner in one block: the units' rows of the sums leave the front launch
            self._call("cvf_ef16_front_transfer", lib.cvf_ef16_front_transfer_rows, *args, P(w), P(w_lag), P(ws.scratch), s)
            return "cvf_ef16_finish", lib.cvf_ef16_finish, lib.cvf_ef16_finish_dp, (self._cfg, ws.B, P(ws.scratch))
        self._call("cvf_ef16_front_transfer", lib.cvf_ef16_front_transfer, *args, s)
        return self._lagged_stats(ws, w, w_lag, lib.cvf_ef_stats_dp)

    def _lagged_stats(self, ws, w, w_lag, fn_dp):
        """The finishing launch of transfer mode: the time-lagged batch sums of ``ws.y``."""
        lib, P = _hip.lib(), _hip.ptr
        y_lag = ws.y[ws.T * self.k * _hip.TILE:]
        return "cvf_ef_stats", lib.cvf_ef_stats, fn_dp, (self._cfg, ws.B, P(w), P(ws.y), None, P(w_lag), P(y_lag), P(ws.scratch))

    def _fwd_fused_gen(self, ws, X, w, X_lag, w_lag, aligned, cache, lv, cf):
        """Generator mode, 64 frames per wave: [alignment,] nets forward, q = J A J^T g, E and the batch sums in one launch (no
        `_dp` twin of its finishing launch: collective #1 and the loss tail follow in their own)."""
        lib, fl, s, P = _hip.lib(), self._flat, _hip.stream(), _hip.ptr
        inside = self._route.align_inside and not aligned
        if not aligned and not inside:
            self._align(ws, ws.slot, X, X_lag)
        name, fn = (("cvf_ef_align_fwd_metric_stats", lib.cvf_ef_align_fwd_metric_stats) if inside else
                    ("cvf_ef_fwd_metric_stats", lib.cvf_ef_fwd_metric_stats))
        rows = lib.cvf_ef_fused_stats_rows(fl.desc, self._pp, ws.B, int(inside))   # > 0: per-tile sums left for a short second launch
        self._call(name, fn, fl.desc, P(fl.theta), P(fl.packed), P(ws.feat), self._pp, P(X), ws.B, P(ws.aux), P(self._diag_coeff),
                   P(ws.y), P(ws.saved), P(ws.q), P(ws.e), self._cfg, P(w), P(ws.scratch), None if rows > 0 else P(ws.stats), lv, cf, s)
        if rows > 0:
            return "cvf_ef_stats_finish_rows", lib.cvf_ef_stats_finish_rows, None, (self._cfg, rows, P(ws.scratch))
        return None

    def _fwd_separate(self, ws, X, w, X_lag, w_lag, aligned, cache, lv, cf):
        """The forward launch and the statistics launch apart: the plain and general routes, and transfer mode of the fused route
        (alignment inside the forward launch).  Neither statistics launch is handed a `_dp` twin here."""
        lib, fl, s, P = _hip.lib(), self._flat, _hip.stream(), _hip.ptr
        gen = self.lag_idx == 0
        inside = self._route.align_inside and not aligned
        if not aligned and not inside:
            self._align(ws, ws.slot, X, X_lag)
        if inside:
            self._call("cvf_ef_align_fwd", lib.cvf_ef_align_fwd, fl.desc, P(fl.theta), P(fl.packed), P(ws.feat), self._pp, P(X),
                       P(X_lag), ws.B, P(ws.y), P(ws.saved), s)
        elif self._route.shared is not None and not gen:
            self._call("cvf_ef_general_shared_transfer_fwd", lib.cvf_ef_general_shared_transfer_fwd, fl.desc, self._route.shared,
                       P(fl.theta), P(ws.feat), ws.Tt, P(ws.y), P(ws.saved), s)
        elif self._route.shared is not None:
            self._call("cvf_ef_general_shared_fwd", lib.cvf_ef_general_shared_fwd, fl.desc, self._route.shared, P(fl.theta), P(ws.feat),
                       ws.Tt, P(ws.y), P(ws.g), P(ws.saved), s)
        elif self._route.kind == "general":
            self._call("cvf_ef_general_fwd", lib.cvf_ef_general_fwd, fl.desc, P(fl.theta), P(ws.feat), ws.Tt, P(ws.y), P(ws.g), P(ws.saved), s)
        else:
            self._call("cvf_ef_mlp_fwd", lib.cvf_ef_mlp_fwd, fl.desc, P(fl.theta), P(fl.packed), P(ws.feat), ws.Tt, P(ws.y), P(ws.g),
                       P(ws.saved), s)
        if not gen:
            return self._lagged_stats(ws, w, w_lag, None)
        # q = J A J^T g, E, and the batch sums (K2/K3 + K5) in one launch
        return "cvf_metric_apply", lib.cvf_metric_apply_stats, None, (
            self._pp, P(X), ws.B, P(ws.aux), P(self._diag_coeff), self.k, P(ws.g), P(ws.q), P(ws.e), P(ws.k1_scratch), P(self._dense),
            self._cfg, P(w), P(ws.y), P(ws.scratch))

    def _backward(self, ws, w, w_lag=None, advance=False, fuse_adam=False):
        """Parameter gradient into the flat buffer.  ``advance``: this gradient belongs to an optimiser step
        (the kernel advances the device step counter).  ``fuse_adam``: single-process training - the kernel
        that sums the per-block partial gradients applies the Adam update in the same launch."""
        lib, fl, P = _hip.lib(), self._flat, _hip.ptr
        name, packed, lagged, q = self._route.backward
        if self._route.shared is not None and self.lag_idx != 0:   # (transfer mode: no q)
            self._call("cvf_ef_general_shared_transfer_backward", lib.cvf_ef_general_shared_transfer_backward, self._cfg, fl.desc,
                       self._route.shared, P(fl.theta), ws.B, P(w), P(w_lag), P(ws.feat_in), P(ws.y), P(ws.coef), P(ws.slab),
                       P(self.optimizer.step_count) if advance else None, P(ws.saved), _hip.stream())
        elif self._route.shared is not None:   # (generator mode: no w_lag; n_shared follows the description)
            self._call("cvf_ef_general_shared_backward", lib.cvf_ef_general_shared_backward, self._cfg, fl.desc, self._route.shared,
                       P(fl.theta), ws.B, P(w), P(ws.feat_in), P(ws.y), P(ws.q), P(ws.coef), P(ws.slab),
                       P(self.optimizer.step_count) if advance else None, P(ws.saved), _hip.stream())
        else:
            self._call(name, getattr(lib, name), self._cfg, fl.desc, P(fl.theta), *([P(fl.packed)] if packed else []), ws.B, P(w),
                       *([P(w_lag)] if lagged else []), P(ws.feat_in), P(ws.y), *([P(ws.q)] if q else []), P(ws.coef), P(ws.slab),
                       P(self.optimizer.step_count) if advance else None, P(ws.saved), _hip.stream())
        local = self._local_only or self._grad_local
        # (the general route's gradient exceeds the peer-to-peer window of cvf_slab_reduce_dp: slab reduction + all-reduce)
        comm = None if local or self._route.kind == "general" else _dist.fused_comm()
        if comm is not None:   # sum of the slab rows -> collective #2 -> (train_step) the identical Adam update: one launch
            adam = self.optimizer.fused_args() if advance else None
            self._call("cvf_slab_reduce_dp", lib.cvf_slab_reduce_dp, P(ws.slab), ws.slab_rows, fl.n, P(fl.grad), adam, comm, _hip.stream())
            return adam is not None
        adam = self.optimizer.fused_args() if fuse_adam else None
        self._call("cvf_slab_reduce", lib.cvf_slab_reduce, P(ws.slab), ws.slab_rows, fl.n, P(fl.grad), adam, _hip.stream())
        if not fuse_adam and not local:
            self._allreduce("allreduce_gradient", fl.grad)                                                # collective #2
        return adam is not None

    def train_step(self, X, w, X_lag=None, w_lag=None, slot=0, aligned=False, prefetch=None, out=None):
        """One optimisation step on device tensors; returns the device vector
        ``[loss, npl, pen, eig_1..k, cvec_1..k]`` (fp64) without synchronising the host.
        ``prefetch = (X_next, X_lag_next)``: align that batch into the other feature buffer on a side stream while this
        step's backward kernel runs; the next call then passes ``slot ^ 1, aligned=True``."""
        ws = self._forward(X, w, X_lag, w_lag, slot, aligned, out=out, cache=True)
        if prefetch is not None:   # beside the backward kernel, which leaves SIMD slots and LDS free at these sizes
            self._side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(self._side):
                self._align(ws, slot ^ 1, prefetch[0], prefetch[1])
        fused = self._backward(ws, w, w_lag, advance=True, fuse_adam=not _dist.collectives())
        if not fused:
            self.optimizer.step(advance=False)
        if prefetch is not None:
            torch.cuda.current_stream().wait_stream(self._side)
        return ws.loss_out

    # -- hipGraph replay of a whole step: batches are static (shuffle=False, core.py:472-481), so every
    #    (batch, kind) pair is captured once and replayed in all later epochs: one host call per step
    def _graph_step(self, key, fn, out_slot, takes_out=False):
        """Run ``fn()`` (a step that returns the device loss vector) and copy its result into ``out_slot``;
        through :meth:`_graph_call`: captured into a hipGraph on first use when graphs are enabled."""
        def run():
            # (steps that take the slot write their loss vector there themselves; others return a tensor to copy)
            got = fn(out_slot) if takes_out else fn()
            if got is not out_slot and got.data_ptr() != out_slot.data_ptr():
                out_slot.copy_(got)

        self._graph_call(key, run)

    def _graph_call(self, key, body):
        """Run ``body()`` - any sequence of steps on static batches that writes its results into fixed device buffers, e.g.
        a whole epoch - through ONE hipGraph: captured on first use (after an eager run that allocates the workspaces),
        replayed afterwards.  One replay per epoch instead of one per step: the ~9 us the GPU idles between two graph
        launches (rocprofv3 kernel trace of bench.py) is paid once per epoch.

        A replay does not pass through Python: the captured steps assume static batch POINTERS and, since they start from
        the batches' alignment rows (:meth:`_alignment_rows`; the ``_version`` check cannot run in a replay), static batch
        CONTENTS.  train() owns its gathered copies; a caller that rewrites a batch in place calls :meth:`drop_alignment_cache`,
        which drops the captured graphs with the rows."""
        if not self._use_graphs:
            body()
            return
        g = self._graphs.get(key)
        if g is None:
            body()                                     # eager: allocates the workspaces (and does this call's work)
            torch.cuda.current_stream().synchronize()
            self.optimizer.sync_lr()
            # unreachable tasks of the same process may still hold captured graphs; the cycle collector would destroy them whenever
            # it next runs - inside the capture below that aborts the process (a graph may not be destroyed while a stream captures)
            gc.collect()
            g = torch.cuda.CUDAGraph()
            try:
                with torch.cuda.graph(g):
                    body()
            except Exception as exc:                   # e.g. a collective that cannot be captured on this stack
                if not _dist.collectives():
                    raise
                self._use_graphs = False
                self._graphs.clear()
                torch.cuda.synchronize()
                print(f"[colvarsfinder] hipGraph capture of the data-parallel steps failed ({type(exc).__name__}: {exc}); "
                      "continuing with eager launches", flush=True)
                return
            self._graphs[key] = g
            return
        self.optimizer.sync_lr()                       # the captured kernels read the learning rate from a device scalar
        g.replay()

    def loss_func(self, X, weight, X_lagged, weight_lagged):
        """core.py:387-457.  Returns ``(loss, eig_vals, non_penalty_loss, penalty, cvec)``; the parameter
        gradient of ``loss`` is obtained with :meth:`backward` (there is no autograd graph)."""
        X, weight = self._dev(X), self._dev(weight)
        X_lagged, weight_lagged = self._dev(X_lagged), self._dev(weight_lagged)
        if self._foreign_pp:   # coordinates, as in the reference: this batch's records / features, then the same kernels
            X = self._frames(X)
            X_lagged = None if X_lagged is None else self._frames(X_lagged)
        self._flat.repack()  # the caller may have modified the parameters through the nn.Module
        ws = self._forward(X, weight, X_lagged, weight_lagged)
        self._last = (ws, weight, weight_lagged)
        v = ws.loss_vec.cpu()
        _dist.check_comm()
        k = self.k
        dt = torch.get_default_dtype()
        cvec = v[3 + k:3 + 2 * k].round().to(torch.long).numpy()
        return v[0].to(dt), v[3:3 + k].to(dt), v[1].to(dt), v[2].to(dt), cvec

    def backward(self):
        """Parameter gradient of the last :meth:`loss_func` call -> ``p.grad`` of the model's parameters."""
        ws, w, w_lag = self._last
        self._backward(ws, w, w_lag)
        super().backward()

    # ---------------------------------------------------------------- training loop
    def train(self):
        """core.py:459-566 with the trajectory resident in HBM and one host copy of the losses per epoch."""
        k, lag = self.k, self.lag_idx
        self._flat.repack()
        self.drop_alignment_cache()   # captured steps hold pointers into the previous call's batches, the rows belong to them
        # core.py:465 (drawn, discarded), core.py:468
        idx_train, idx_test = _agreed_split(self._n_frames - lag, self.test_ratio, 2, self.device)

        def resident(idx, bs):
            """Frames (weights, lagged partners) of the permuted set `idx` that this process works on, gathered once in
            batch order, and its batches as row ranges of that copy: DataLoader(batch_size=bs, drop_last=True,
            shuffle=False), core.py:470-481.  One process: the whole set (the tail drop_last discards included), gathered on
            the device from the resident trajectory.  Data-parallel: only this rank's slice of every global batch
            (_static_batches), gathered on the host and uploaded - the lagged partners are pre-gathered too, so a frame
            may live on two ranks."""
            pos, _, bl = _static_batches(len(idx), bs)
            rows = np.asarray(idx)[pos]
            it = torch.as_tensor(rows, device=self.device, dtype=torch.long)
            w, wl = self._weights[it].contiguous(), self._weights[it + lag].contiguous() if lag > 0 else None
            if not self._sharded:
                X, Xl = self._traj[it].contiguous(), self._traj[it + lag].contiguous() if lag > 0 else None
            else:
                X = _hip.upload_f32(self._traj_host.rows(rows), self.device)
                Xl = _hip.upload_f32(self._traj_host.rows(rows + lag), self.device) if lag > 0 else None
            self.resident_bytes += sum(t.numel() * t.element_size() for t in (X, w, Xl, wl) if t is not None)
            return (X, w, Xl, wl), bl

        bs_train = min(self.batch_size, len(idx_train))
        bs_test = min(self.batch_size, len(idx_test))
        self.resident_bytes = 0 if self._sharded else self._traj.numel() * 4
        Xtr, tr_batches = resident(idx_train, bs_train)
        Xte, te_batches = resident(idx_test, bs_test)

        self.loss_list = []
        min_loss = float("inf")
        self._announce((bs_train, bs_test), (len(idx_train), len(idx_test)), (len(tr_batches), len(te_batches)))
        loss_names = ['loss', 'eigen_non_penalty', 'eigen_penalty'] + ['eig_%d' % (i + 1) for i in range(k)]
        log_tr, log_te = self._epoch_logs(len(tr_batches), len(te_batches), 3 + 2 * k)

        def sl(data, a, b):
            return tuple(None if t is None else t[a:b] for t in data)

        def on_epoch(ep, tr, te):
            """Host side of one finished epoch: loss_list (core.py:553), _cvec (core.py:515), the writer (core.py:559-561)."""
            dt = torch.get_default_dtype()
            if len(tr_batches) > 0:
                self._cvec = tr[-1, 3 + k:].round().to(torch.long).numpy()
            self.loss_list.append([tr[:, :3 + k].to(dt), te[:, :3 + k].to(dt)])
            self._write_epoch_means(loss_names, ep, *self.loss_list[-1])

        elog = _AsyncEpochLog(log_tr, log_te, len(tr_batches), len(te_batches), on_epoch)

        def train_one(it):
            X, w, Xl, wl = sl(Xtr, *tr_batches[it])
            nxt = None
            if self._pipeline and it + 1 < len(tr_batches):
                Xn, _, Xln, _ = sl(Xtr, *tr_batches[it + 1])
                nxt = (Xn, Xln)
            self.train_step(X, w, Xl, wl, slot=it % 2, aligned=self._pipeline and it > 0, prefetch=nxt, out=log_tr[it])

        def test_one(it):                                          # core.py:535-551 (same loss, no update)
            X, w, Xl, wl = sl(Xte, *te_batches[it])
            self._forward(X, w, Xl, wl, out=log_te[it], cache=True)

        # every step of the epoch (static batches) replays from hipGraphs: ONE graph per epoch, or - small batches on a long
        # trajectory - one per kEpochChunk steps (a graph of many thousands of kernel nodes takes seconds to instantiate)
        kEpochChunk = 256
        steps = [(train_one, it) for it in range(len(tr_batches))] + [(test_one, it) for it in range(len(te_batches))]
        chunks = [steps[c:c + kEpochChunk] for c in range(0, len(steps), kEpochChunk)]

        for epoch in _tqdm(range(self.num_epochs), disable=(_dist.rank() != 0)):
            self.model.train()
            for ci, chunk in enumerate(chunks):
                self._graph_call(("epoch", ci), lambda chunk=chunk: [fn(it) for fn, it in chunk])
            elog.push(epoch)        # (the host reads the epoch's numbers later; epochs that save or plot flush first)
            saving, plotting = self._due(epoch)
            if saving or plotting:
                elog.flush_all()
            if saving:
                last = float(self.loss_list[-1][0][-1, 0]) if len(tr_batches) > 0 else float("inf")
                min_loss = self._save_latest_and_best(epoch, last, min_loss)
            if plotting:
                self._plot(epoch)
        elog.flush_all()
        self._loss_frames(loss_names)


class AutoEncoderTask(TrainingTask):
    """Autoencoder trained with the weighted reconstruction loss (arguments as core.py:610-625).

    The feature trajectory ``r(x)`` is computed once for all frames (core.py:635) by kernel K1 and
    stays in HBM; each step is one fused kernel (forward, weighted MSE, parameter gradient) + Adam.  Chains whose parameters
    and activations do not fit that kernel's 160 KiB of LDS train layer by layer instead (cvf_ae_general_step: any widths up
    to 4096 units, the same outputs); a chain past both routes is refused with NotImplementedError at construction.
    """

    def __init__(self, traj_obj, pp_layer, model, model_path, learning_rate=0.01, load_model_filename=None,
                 save_model_every_step=10, batch_size=1000, num_epochs=10, test_ratio=0.2, optimizer_name='Adam',
                 device=torch.device('cuda'), plot_class=None, plot_frequency=0, verbose=True, debug_mode=True):
        super().__init__(traj_obj, pp_layer, model, model_path, learning_rate, load_model_filename, save_model_every_step,
                         model.encoded_dim, batch_size, num_epochs, test_ratio, optimizer_name, device, plot_class,
                         plot_frequency, verbose, debug_mode)
        assert isinstance(model, AutoEncoder), 'model must be an object of the class AutoEncoder'
        self.init_model_and_optimizer()
        self._traj_host = _HostFrames(traj_obj.trajectory)
        self._n_frames = int(self._traj_host.shape[0])
        self._weights = torch.as_tensor(np.asarray(traj_obj.weights)).to(device=self.device, dtype=torch.float32).contiguous()
        # pp_layer: the alignment + feature kernel (AlignFeatureLayer / Identity) or ANY torch module (core.py:65,122,635): this
        # task applies it exactly once, to build the feature trajectory - a foreign module is run there with torch, on the
        # device, and the training step (cvf_ae_step on the resident feature rows) is the same either way
        self._foreign_pp = not isinstance(self.preprocessing_layer, (torch.nn.Identity, AlignFeatureLayer))
        self._pp = pp = (self._probe_pp(self._traj_host.rows(np.arange(1))) if self._foreign_pp else
                         self._pp_desc(int(np.prod(self._traj_host.shape[1:]))))
        # core.py:635: the feature trajectory r(x) of ALL frames, once.  In a data-parallel job (one process per GPU) each
        # rank computes the features of its own rows only, in train(), once the split is known.
        self._sharded = _dist.world() > 1
        self._feature_traj = None if self._sharded else self._features(self._traj_host.all())
        self.resident_bytes = 0 if self._sharded else self._feature_traj.numel() * 4
        assert pp.d_r == self._flat.desc.dims[0] == self._flat.desc.dims[self._flat.desc.n_layers], \
            'autoencoder input/output width must equal the feature dimension'
        if self.verbose:
            print('\nShape of trajectory data array:\n {}'.format((self._n_frames, pp.d_r)), flush=True)
        self._out2 = torch.zeros(3, device=self.device, dtype=torch.float64)
        self._scratch = {}
        # with_grad -> the step goes per layer (cvf_ae_general_step): decided once, where cvf_ae_step_route refuses the chain
        self._general = {wg: self._needs_general(wg) for wg in (False, True)}

    def _needs_general(self, with_grad):
        """False where cvf_ae_step takes the chain (its kernels keep the chain of a 64-frame tile in LDS), True where only the
        per-layer route of csrc/ae_general.hip does; a chain past both is refused here, at construction."""
        lib, fl = _hip.lib(), self._flat
        if lib.cvf_ae_step_route(fl.desc, _hip.ptr(fl.theta), int(with_grad), None) >= 0:
            return False
        fused = lib.cvf_last_error().decode()
        if lib.cvf_ae_general_supported(fl.desc) != 1:
            raise NotImplementedError("AutoEncoderTask: no HIP route trains this chain (%s; %s)"
                                      % (fused, lib.cvf_last_error().decode()))
        return True

    def colvar_model(self):
        """core.py:640-647."""
        return _CVModel(self.preprocessing_layer, self.model.encoder, device=self.device)

    def reg_model(self):
        return None

    def _step(self, feat, idx, w, with_grad, inv_wsum=None, advance=False, fuse_adam=False):
        """One fused kernel: forward, weighted MSE, parameter gradient (+ Adam when ``fuse_adam``).
        ``inv_wsum`` = 1 / (global sum of the batch weights); it does not depend on the model, so ``train``
        computes it once per (static) batch."""
        lib, fl = _hip.lib(), self._flat
        B = w.shape[0]
        general = self._general[bool(with_grad)]
        step, name = (lib.cvf_ae_general_step, "cvf_ae_general_step") if general else (lib.cvf_ae_step, "cvf_ae_step")
        sc = self._scratch.get((B, general))
        if sc is None:
            size = lib.cvf_ae_general_scratch_floats if general else lib.cvf_ae_scratch_floats
            sc = self._scratch[(B, general)] = torch.empty(size(fl.desc, B), device=self.device, dtype=torch.float32)
        if inv_wsum is None:
            wsum = w.sum(dtype=torch.float64)
            _dist.allreduce_sum_(wsum)
            inv_wsum = 1.0 / float(wsum)
        adam = self.optimizer.fused_args() if (fuse_adam and with_grad) else None
        _hip.check(step(fl.desc, _hip.ptr(fl.theta), _hip.ptr(feat), _hip.ptr(idx), B, _hip.ptr(w), inv_wsum, _hip.ptr(sc),
                        _hip.ptr(self._out2), _hip.ptr(fl.grad) if with_grad else None,
                        _hip.ptr(self.optimizer.step_count) if advance else None, adam, _hip.stream()), name)
        if _dist.world() == 1:
            # (the kernel left the ratio beside the two sums: no arithmetic launches on the host side of a step; the caller
            #  copies the value out before the next step overwrites it)
            if with_grad and adam is None and advance:
                self.optimizer.step(advance=False)
            return self._out2[2]
        out = self._out2[:2].clone()
        _dist.allreduce_sum_(out)
        if with_grad and adam is None:
            self._allreduce("allreduce_gradient", fl.grad)
            if advance:
                self.optimizer.step(advance=False)
        return out[0] / out[1]

    def weighted_MSE_loss(self, X, weight):
        """core.py:652-666 on a feature batch ``X [B, d_r]``; ``backward()`` afterwards fills ``p.grad``."""
        X = torch.as_tensor(X).detach().to(device=self.device, dtype=torch.float32).contiguous()
        weight = torch.as_tensor(weight).detach().to(device=self.device, dtype=torch.float32).contiguous()
        loss = self._step(X, None, weight, with_grad=True)
        return loss.to(torch.get_default_dtype(), copy=True)

    def train(self):
        """core.py:668-744."""
        idx_train, idx_test = _agreed_split(self._n_frames, self.test_ratio, 1, self.device)   # core.py:672 (one draw)
        bs_train, bs_test = min(self.batch_size, len(idx_train)), min(self.batch_size, len(idx_test))

        def resident(idx, bs):
            """(feature rows, per-batch row indices or None, weights, batches) of the permuted set `idx` for this process.
            One process: batches index the resident feature trajectory.  Data-parallel: only this rank's slice of every
            global batch is uploaded and run through K1 (_static_batches); its batches are contiguous row ranges."""
            pos, _, bl = _static_batches(len(idx), bs)
            rows = np.asarray(idx)[pos]
            it = torch.as_tensor(rows, device=self.device, dtype=torch.long)
            if not self._sharded:
                return self._feature_traj, it, self._weights[it].contiguous(), bl
            feat = self._features(self._traj_host.rows(rows))
            self.resident_bytes += feat.numel() * 4
            return feat, None, self._weights[it].contiguous(), bl

        if self._sharded:
            self.resident_bytes = 0
        ftr, itr, wtr, tr_batches = resident(idx_train, bs_train)
        fte, ite, wte, te_batches = resident(idx_test, bs_test)
        if self._sharded:
            self._feature_traj = ftr      # (this rank's training rows; the reference's attribute holds all frames)

        def rows_of(feat, it, a, b):
            return (feat, it[a:b]) if it is not None else (feat[a:b], None)

        iw_tr = [1.0 / v for v in _batch_weight_sums(wtr, tr_batches)]
        iw_te = [1.0 / v for v in _batch_weight_sums(wte, te_batches)]
        self.loss_list = []
        min_loss = float("inf")
        self._announce((bs_train, bs_test), (len(idx_train), len(idx_test)), (len(tr_batches), len(te_batches)))
        log_tr, log_te = self._epoch_logs(len(tr_batches), len(te_batches))

        def on_epoch(ep, tr, te):
            dt = torch.get_default_dtype()
            tr, te = tr.to(dt), te.to(dt)
            self.loss_list.append([tr, te])                                        # core.py:736
            self.writer.add_scalar('Loss/train', tr.mean() if len(tr) else float("nan"), ep)   # core.py:738-739
            self.writer.add_scalar('Loss/test', te.mean() if len(te) else float("nan"), ep)

        elog = _AsyncEpochLog(log_tr, log_te, len(tr_batches), len(te_batches), on_epoch)
        fuse_adam = _dist.world() == 1
        for epoch in _tqdm(range(self.num_epochs), disable=(_dist.rank() != 0)):
            self.model.train()
            for it, (a, b) in enumerate(tr_batches):
                log_tr[it] = self._step(*rows_of(ftr, itr, a, b), wtr[a:b], True, iw_tr[it], advance=True, fuse_adam=fuse_adam)
            self.model.eval()
            for it, (a, b) in enumerate(te_batches):
                log_te[it] = self._step(*rows_of(fte, ite, a, b), wte[a:b], False, iw_te[it])
            elog.push(epoch)
            saving, plotting = self._due(epoch)
            if saving or plotting:
                elog.flush_all()
            if saving:
                last = float(self.loss_list[-1][0][-1]) if len(tr_batches) else float("inf")
                min_loss = self._save_latest_and_best(epoch, last, min_loss)
            if plotting:
                self._plot(epoch)
        elog.flush_all()
        self._loss_frames(['loss'])


# ----------------------------------------------------------------------------------------------------------------------
# RegAutoEncoderTask (core.py:746-1217)
# ----------------------------------------------------------------------------------------------------------------------
class _RegFlatParams:
    """A :class:`RegAutoEncoder` as ONE chain over a flat fp32 buffer: the encoder's layers, then the decoder and
    the K regulariser nets side by side.  Merged layer m maps ``[dec_m | reg_1,m | .. | reg_K,m]`` to the same of
    m + 1 with a block-structured matrix (the first one: every block reads the whole latent vector), so the last
    layer emits ``[reconstruction | y_1..y_K]`` and one pass of the chain kernel serves ``forward_ae`` and
    ``forward_reg`` (nn.py:174-198).  Every module parameter aliases its block of the buffer (a strided view for the
    block-diagonal layers); ``mask`` is 1 on real parameters, 0 on structural zeros and frozen (encoder) entries.
    """

    def __init__(self, model, device, freeze_encoder=False):
        from .nn import _chain_layers
        model.to(device=device, dtype=torch.float32)
        enc, dec = _chain_layers(model.encoder), _chain_layers(model.decoder)
        regs = [_chain_layers(r) for r in model.reg] if model.num_reg > 0 else []
        K, Ld = len(regs), len(dec)
        for r in regs:
            if len(r) != Ld or any(ra != da for (_, ra), (_, da) in zip(r, dec)):
                raise NotImplementedError("this layout runs decoder and regulariser nets side by side, layer for layer: they must have "
                                          "the same number of layers and activations (nets of different depths take "
                                          "_RegRaggedFlatParams and the cvf_regae_ragged_* calls, as RegAutoEncoderTask chooses)")
            if r[-1][0].out_features != 1:
                raise NotImplementedError("regulariser nets must be scalar-valued")
        assert len(enc) + Ld <= _hip.MAX_LAYERS, f"at most {_hip.MAX_LAYERS} layers (encoder + decoder)"
        # sizes
        shapes = [(lin.out_features, lin.in_features, act) for lin, act in enc]
        for m in range(Ld):
            fin = dec[m][0].in_features if m == 0 else dec[m][0].in_features + sum(r[m][0].in_features for r in regs)
            fout = dec[m][0].out_features + sum(r[m][0].out_features for r in regs)
            shapes.append((fout, fin, dec[m][1]))
        self.n = sum(fo * fi + fo for fo, fi, _ in shapes)
        self.theta = torch.zeros(self.n, device=device, dtype=torch.float32)
        self.grad = torch.zeros(self.n, device=device, dtype=torch.float32)
        self.mask = torch.zeros(self.n, device=device, dtype=torch.float32)
        self.packed = None
        self.K = K
        d = _hip.MLPDesc()
        d.n_nets, d.n_layers, d.n_params = 1, len(shapes), self.n
        self.views = []   # (parameter, view of theta, view of grad)

        def alias(p, region, r0, r1, c0=None, c1=None, frozen=False):
            tv = region(self.theta)[r0:r1] if c0 is None else region(self.theta)[r0:r1, c0:c1]
            gv = region(self.grad)[r0:r1] if c0 is None else region(self.grad)[r0:r1, c0:c1]
            mv = region(self.mask)[r0:r1] if c0 is None else region(self.mask)[r0:r1, c0:c1]
            tv.copy_(p.data)
            mv.fill_(0.0 if frozen else 1.0)
            p.data = tv
            self.views.append((p, tv, gv))

        pos = 0
        for l, (fo, fi, act) in enumerate(shapes):
            d.dims[l], d.dims[l + 1], d.act[l] = fi, fo, int(act)
            d.w_off[0][l], d.b_off[0][l] = pos, pos + fo * fi
            wreg = (lambda t, a=pos, fo=fo, fi=fi: t[a:a + fo * fi].view(fo, fi))
            breg = (lambda t, a=pos + fo * fi, fo=fo: t[a:a + fo])
            if l < len(enc):
                lin = enc[l][0]
                alias(lin.weight, wreg, 0, fo, 0, fi, frozen=freeze_encoder)
                alias(lin.bias, breg, 0, fo, frozen=freeze_encoder)
            else:
                m = l - len(enc)
                r0 = c0 = 0
                for chain in [dec] + regs:
                    lin = chain[m][0]
                    cw = lin.in_features
                    if m == 0:
                        alias(lin.weight, wreg, r0, r0 + lin.out_features, 0, cw)       # every block reads the latent vector
                    else:
                        alias(lin.weight, wreg, r0, r0 + lin.out_features, c0, c0 + cw)
                        c0 += cw
                    alias(lin.bias, breg, r0, r0 + lin.out_features)
                    r0 += lin.out_features
            pos += fo * fi + fo
        self.desc = d

    def repack(self):
        pass

    def grad_views(self):
        return [(p, gv) for p, _, gv in self.views]


class _RegRaggedFlatParams(_RegFlatParams):
    """:class:`_RegFlatParams` for a decoder of ``Ld`` and regulariser nets of ``Lr != Ld`` Linear layers (``n_dec`` / ``n_reg``): the
    chain of ``cvf_regae_ragged_*`` (include/cvf.h), ``n_enc + max(Ld, Lr)`` layers.  Merged layer m holds the rows of the groups
    still alive at depth m, the deeper group's first (``dec_deep``: ``[dec_m | reg_1,m | .. | reg_K,m]``, else the K nets and then
    the decoder).  The shallower group's last layer has no activation and its rows stay in that layer's image; the next layer
    reads the rows before them, so its matrix is dense ``[out][live rows]`` - no column is ever stored for a finished row.  The
    chain ends in the deeper group's outputs.  Aliasing, ``mask`` and ``grad_views`` are :class:`_RegFlatParams`'s."""

    def __init__(self, model, device, freeze_encoder=False):
        from .nn import _chain_layers
        model.to(device=device, dtype=torch.float32)
        enc, dec = _chain_layers(model.encoder), _chain_layers(model.decoder)
        regs = [_chain_layers(r) for r in model.reg]
        K, Ld, Lr = len(regs), len(dec), len(regs[0])
        assert K > 0 and Ld != Lr, "equal depths are _RegFlatParams's"
        for r in regs:
            if [(lin.in_features, lin.out_features, a) for lin, a in r] != [(lin.in_features, lin.out_features, a) for lin, a in regs[0]]:
                raise NotImplementedError("the regulariser nets must share one reg_layer_dims and one activation")
            if r[-1][0].out_features != 1:
                raise NotImplementedError("regulariser nets must be scalar-valued")
        self.dec_deep = Ld > Lr
        deep, shallow = ([dec], regs) if self.dec_deep else (regs, [dec])
        Ls, Lmax = min(Ld, Lr), max(Ld, Lr)
        # the two groups run through the same epilogue up to the layer that ends the shallower one, whose rows take none
        if any(shallow[0][m][1] != deep[0][m][1] for m in range(Ls - 1)) or shallow[0][Ls - 1][1] != 0:
            raise NotImplementedError("decoder and regulariser nets of different depths (csrc/regae_general.hip: cvf_regae_ragged_*) "
                                      "must share the activation between their layers and have none behind their last ones")
        assert len(enc) + Lmax <= _hip.MAX_LAYERS, f"at most {_hip.MAX_LAYERS} layers (encoder + the deeper of decoder and regulariser nets)"
        self.n_dec, self.n_reg, self.K = Ld, Lr, K
        alive = lambda m: deep + (shallow if m < Ls else [])
        shapes = [(lin.out_features, lin.in_features, act) for lin, act in enc]
        for m in range(Lmax):
            fin = dec[0][0].in_features if m == 0 else sum(ch[m][0].in_features for ch in alive(m))
            shapes.append((sum(ch[m][0].out_features for ch in alive(m)), fin, deep[0][m][1]))
        self.n = sum(fo * fi + fo for fo, fi, _ in shapes)
        self.theta = torch.zeros(self.n, device=device, dtype=torch.float32)
        self.grad = torch.zeros(self.n, device=device, dtype=torch.float32)
        self.mask = torch.zeros(self.n, device=device, dtype=torch.float32)
        self.packed = None
        d = _hip.MLPDesc()
        d.n_nets, d.n_layers, d.n_params = 1, len(shapes), self.n
        self.views = []   # (parameter, view of theta, view of grad)

        def alias(p, region, r0, r1, c0=None, c1=None, frozen=False):
            tv, gv, mv = (region(t)[r0:r1] if c0 is None else region(t)[r0:r1, c0:c1] for t in (self.theta, self.grad, self.mask))
            tv.copy_(p.data)
            mv.fill_(0.0 if frozen else 1.0)
            p.data = tv
            self.views.append((p, tv, gv))

        pos = 0
        d.dims[0] = shapes[0][1]
        for l, (fo, fi, act) in enumerate(shapes):
            d.dims[l + 1], d.act[l] = fo, int(act)      # (dims[l] is the image's width: fi + the finished rows behind a live prefix)
            d.w_off[0][l], d.b_off[0][l] = pos, pos + fo * fi
            wreg = (lambda t, a=pos, fo=fo, fi=fi: t[a:a + fo * fi].view(fo, fi))
            breg = (lambda t, a=pos + fo * fi, fo=fo: t[a:a + fo])
            if l < len(enc):
                lin = enc[l][0]
                alias(lin.weight, wreg, 0, fo, 0, fi, frozen=freeze_encoder)
                alias(lin.bias, breg, 0, fo, frozen=freeze_encoder)
            else:
                m = l - len(enc)
                r0 = c0 = 0
                for chain in alive(m):
                    lin = chain[m][0]
                    cw = lin.in_features
                    if m == 0:
                        alias(lin.weight, wreg, r0, r0 + lin.out_features, 0, cw)       # every block reads the latent vector
                    else:
                        alias(lin.weight, wreg, r0, r0 + lin.out_features, c0, c0 + cw)
                        c0 += cw
                    alias(lin.bias, breg, r0, r0 + lin.out_features)
                    r0 += lin.out_features
            pos += fo * fi + fo
        self.desc = d


class _EncGradPenalty:
    """``eta[0]``: ``reg_enc_grad_loss`` (core.py:896-910) = sum_i (1/W) sum_b w_b |d enc_i / d r (r_b)|^2, the derivative
    taken with respect to the FEATURES r = pp(x) (``Y.requires_grad_()`` there), and its gradient with respect to the
    encoder's parameters (second order through the encoder).

    That is the energy term of the eigenfunction task's generator mode with an identity preprocessing layer and
    ``diag_coeff = 1``, for k "virtual" scalar nets that share the encoder's hidden layers and end in row i of its last layer.
    So it runs on the eigenfunction kernels: the encoder's parameters are gathered into the k-net layout, ``cvf_ef_mlp_fwd``
    (y, g = dy/dr) + ``cvf_metric_apply_stats`` (E_i = |g_i|^2 and the batch sums) give the term, ``cvf_ef_backward`` with the
    coefficient vector [0 .. eta_0 / W on the E entries .. 0] + ``cvf_slab_reduce`` give d(eta_0 term)/d(virtual parameters), and
    the k copies of the shared layers are added back (fixed order) into the encoder's block of the flat gradient.

    ``RegAutoEncoderTask(general_nets=True)`` and an encoder without such an instance (any hidden widths up to 4096, 1 to 11
    hidden layers): the shared-trunk launches of csrc/ef_general.hip (``cvf_ef_general_shared_fwd`` / ``_backward``, DESIGN.md
    section 4.12) in place of ``cvf_ef_mlp_fwd`` / ``cvf_ef_backward``.  The k virtual nets are described IN PLACE over the
    encoder's block of the task's flat buffer - hidden layers shared, net i's output layer = row i of the last weight and entry i
    of the last bias - so nothing is gathered, and the gradient of that block comes back as one vector."""

    def __init__(self, task):
        from .nn import _chain_layers
        enc = _chain_layers(task.model.encoder)
        self.task, self.k, self.L = task, task.k, len(enc)
        fl, dev, k, L = task._flat, task.device, task.k, len(enc)
        dims = [enc[0][0].in_features] + [lin.out_features for lin, _ in enc]
        assert dims[0] == task.tot_dim, \
            (f"eta[0] > 0: the gradient-norm penalty reshapes the encoder's input gradient to [-1, {task.tot_dim}] (core.py:907), "
             f"so the preprocessing layer must emit {task.tot_dim} features, not {dims[0]}")
        act0 = enc[0][1] if L >= 2 else 0
        if L < 2 or act0 == 0 or [a for _, a in enc] != [act0] * (L - 1) + [0]:
            raise NotImplementedError("eta[0] on MI355X: the encoder must be Linear + activation layers (one activation) ending in a Linear layer")
        d = _hip.MLPDesc()
        vd = dims[:-1] + [1]
        d.n_nets, d.n_layers = k, L
        for l in range(L):
            d.dims[l], d.dims[l + 1], d.act[l] = vd[l], vd[l + 1], (act0 if l < L - 1 else 0)
        # virtual net i = [shared layers 0..L-2 | row i of the last weight | entry i of the last bias]
        ed = fl.desc
        n_shared = ed.w_off[0][L - 1] - ed.w_off[0][0]
        assert ed.w_off[0][0] == 0 and ed.b_off[0][L - 2] + dims[L - 1] == n_shared   # the encoder opens the flat buffer
        h = dims[L - 1]
        per = n_shared + h + 1
        src, pos = [], 0
        for i in range(k):
            for l in range(L - 1):
                d.w_off[i][l], d.b_off[i][l] = pos + ed.w_off[0][l], pos + ed.b_off[0][l]
            d.w_off[i][L - 1], d.b_off[i][L - 1] = pos + n_shared, pos + n_shared + h
            src += list(range(n_shared)) + list(range(ed.w_off[0][L - 1] + i * h, ed.w_off[0][L - 1] + (i + 1) * h)) + [ed.b_off[0][L - 1] + i]
            pos += per
        d.n_params = pos
        n_pack = _hip.lib().cvf_ef_pack_floats(d) if k <= _hip.MAX_NETS else 0
        self.shared = None
        if n_pack <= 0 and task.general_nets:   # no instance: the nets in place, on the shared-trunk launches
            for i in range(k):
                for l in range(L - 1):
                    d.w_off[i][l], d.b_off[i][l] = ed.w_off[0][l], ed.b_off[0][l]
                d.w_off[i][L - 1], d.b_off[i][L - 1] = ed.w_off[0][L - 1] + i * dims[L - 1], ed.b_off[0][L - 1] + i
            d.n_params = pos = ed.b_off[0][L - 1] + k       # the encoder's block of the flat buffer
            if not _hip.lib().cvf_ef_general_shared_supported(d, L - 1):
                raise NotImplementedError(f"eta[0] on MI355X (general_nets=True), encoder widths {dims}: "
                                          f"{_hip.lib().cvf_last_error().decode()}")
            self.shared = L - 1
        elif n_pack <= 0:
            raise NotImplementedError(
                f"eta[0] on MI355X runs on the eigenfunction kernels: encoder widths {dims} need 1 to 3 equal hidden layers of one of "
                f"{_hip.EF_HIDDEN_WIDTHS} units and at most {_hip.MAX_NETS} latent components (pass general_nets=True to "
                "RegAutoEncoderTask for other encoders: the shared-trunk kernels of csrc/ef_general.hip)")
        self.desc, self.n, self.per, self.n_shared, self.h = d, pos, per, n_shared, h
        self.last_w, self.last_b = int(ed.w_off[0][L - 1]), int(ed.b_off[0][L - 1])
        if self.shared is None:
            self.src = torch.tensor(src, device=dev, dtype=torch.long)
            self.theta = torch.zeros(pos, device=dev, dtype=torch.float32)
            self.packed = torch.zeros(n_pack, device=dev, dtype=torch.float32)
        self.grad = torch.zeros(pos, device=dev, dtype=torch.float32)
        self.ones = torch.ones(dims[0], device=dev, dtype=torch.float32)
        self.pp = identity_desc(dims[0])
        cfg = _hip.EFCfg()
        cfg.k, cfg.lag_idx, cfg.sort_eigvals, cfg.alpha, cfg.beta, cfg.dt = k, 0, 0, 0.0, 1.0, 1.0
        for i in range(k):
            cfg.eig_w[i] = 1.0
        self.cfg, self.d_r = cfg, dims[0]
        self._ws = {}

    def _workspace(self, B):
        ws = self._ws.get(B)
        if ws is None:
            lib, k, d_r, dev = _hip.lib(), self.k, self.d_r, self.task.device
            T = _hip.ntiles(B)
            f32, f64 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.float64)
            if self.shared is not None:
                n_saved = lib.cvf_ef_general_shared_saved_floats(self.desc, T, self.shared)
                rows = lib.cvf_ef_general_shared_slab_rows(self.desc, T, self.shared)
            else:
                n_saved = lib.cvf_ef_saved_floats(self.desc, T)
                rows = lib.cvf_ef_backward_slab_rows(T)
            ws = dict(T=T, feat=torch.empty(T * d_r * _hip.TILE, **f32), y=torch.empty(T * k * _hip.TILE, **f32),
                      g=torch.empty(T * k * d_r * _hip.TILE, **f32), q=torch.empty(T * k * d_r * _hip.TILE, **f32),
                      e=torch.empty(T * k * _hip.TILE, **f32),
                      scratch=torch.zeros(lib.cvf_metric_stats_scratch_doubles(B, k), **f64),
                      stats=torch.zeros(lib.cvf_ef_nstats(k, 0), **f64), coef=torch.zeros(4 * k + k * k, **f64),
                      saved=torch.empty(n_saved, **f32) if n_saved > 0 else None, rows=rows,
                      slab=torch.empty(rows * self.n, **f32))
            self._ws[B] = ws
        return ws

    def run(self, rows, w, eta0, with_grad, dp=False):
        """``rows``: [B, d_r] feature rows of the batch (contiguous), ``w``: [B].  Returns the term (0-dim fp64 device tensor);
        with ``with_grad`` adds d(eta0 * term)/d(encoder parameters) to the encoder's block of the task's flat gradient.
        ``dp``: the batch is this rank's slice of a global batch - the batch sums are added across the ranks, the gradient
        contribution stays this rank's share (the caller sums the flat gradient)."""
        task, lib, P, s = self.task, _hip.lib(), _hip.ptr, _hip.stream()
        fl, k = task._flat, self.k
        B = int(rows.shape[0])
        ws = self._workspace(B)
        if self.shared is None:
            torch.index_select(fl.theta, 0, self.src, out=self.theta)
            task._call("cvf_ef_pack", lib.cvf_ef_pack, self.desc, P(self.theta), P(self.packed), s)
        task._call("cvf_align_feature_fwd", lib.cvf_align_feature_fwd, self.pp, P(rows), B, P(ws["feat"]), None, None, None, s)
        if self.shared is not None:   # (the nets read the encoder's block of the flat buffer where it is)
            task._call("cvf_ef_general_shared_fwd", lib.cvf_ef_general_shared_fwd, self.desc, self.shared, P(fl.theta), P(ws["feat"]),
                       ws["T"], P(ws["y"]), P(ws["g"]), P(ws["saved"]), s)
        else:
            task._call("cvf_ef_mlp_fwd", lib.cvf_ef_mlp_fwd, self.desc, P(self.theta), P(self.packed), P(ws["feat"]), ws["T"], P(ws["y"]),
                       P(ws["g"]), P(ws["saved"]), s)
        task._call("cvf_metric_apply", lib.cvf_metric_apply_stats, self.pp, P(rows), B, None, P(self.ones), k, P(ws["g"]), P(ws["q"]),
                   P(ws["e"]), None, None, self.cfg, P(w), P(ws["y"]), P(ws["scratch"]), P(ws["stats"]), None, None, s)
        st = ws["stats"]                                   # [W, S1(k), S2(i<=j), E(k)]
        if dp:
            task._allreduce("allreduce_batch_sums", st)
        e0 = 1 + k + k * (k + 1) // 2
        term = st[e0:e0 + k].sum() / st[0]
        if with_grad:
            ge = ws["coef"][k + k * k:2 * k + k * k]       # [gS1(k), gS2(k*k), gE(k), ...]: d(eta0 term)/dE_i = eta0 / W
            ge.copy_((eta0 / st[0]).expand(k))
            if self.shared is not None:
                task._call("cvf_ef_general_shared_backward", lib.cvf_ef_general_shared_backward, self.cfg, self.desc, self.shared,
                           P(fl.theta), B, P(w), P(ws["feat"]), P(ws["y"]), P(ws["q"]), P(ws["coef"]), P(ws["slab"]), None,
                           P(ws["saved"]), s)
                task._call("cvf_slab_reduce", lib.cvf_slab_reduce, P(ws["slab"]), ws["rows"], self.n, P(self.grad), None, s)
                fl.grad[:self.n] += self.grad     # the encoder's block, its shared layers summed over the nets inside the launch
                return term
            task._call("cvf_ef_backward", lib.cvf_ef_backward, self.cfg, self.desc, P(self.theta), P(self.packed), B, P(w), None,
                       P(ws["feat"]), P(ws["y"]), P(ws["q"]), P(ws["coef"]), P(ws["slab"]), None, P(ws["saved"]), s)
            task._call("cvf_slab_reduce", lib.cvf_slab_reduce, P(ws["slab"]), ws["rows"], self.n, P(self.grad), None, s)
            gv = self.grad.view(k, self.per)
            fl.grad[:self.n_shared] += gv[:, :self.n_shared].sum(0)
            fl.grad[self.last_w:self.last_w + k * self.h].view(k, self.h).add_(gv[:, self.n_shared:self.n_shared + self.h])
            fl.grad[self.last_b:self.last_b + k] += gv[:, self.n_shared + self.h]
        return term


class _RegGenerator:
    """The eigenfunction regulariser in GENERATOR mode (``gamma`` with ``lag_tau_reg = 0``, the constructor's default;
    core.py:990,1008-1022): y_i = reg_i(encoder(r(x))) differentiated with respect to the coordinates x, the same loss as
    :class:`EigenFunctionTask`'s generator mode with ``diag_coeff = 1`` (core.py:851).

    The K chains reg_i o encoder ARE scalar nets d_r -> .. -> 1: the encoder's hidden layers (shared), one merged layer
    (the encoder's last Linear has no activation, so it folds into the regulariser's first: W = W_r1 W_e, b = W_r1 b_e + b_r1),
    the regulariser's remaining layers.  They are laid out as an :class:`EigenFunctions` model of K nets, every hidden layer
    zero-padded to one kernel width, and handed to an inner ``EigenFunctionTask`` - so the step runs on that task's kernels
    (alignment derivative, forward, q = J J^T g, batch sums, loss tail, backward), whichever it picks for the shape.  The
    gradient with respect to the virtual parameters goes back to the module's parameters through the (tiny) map that built
    them, by autograd on the host-side torch graph: shared layers summed over i, the merged layer by the product rule.

    ``RegAutoEncoderTask(general_nets=True)`` and a chain without such a layout (1 to 11 hidden layers of up to 4096 units, any
    of the six activations): the chains are laid out UNPADDED with the trunk - the encoder's hidden layers - stored once
    (:class:`_SharedTrunkFlat`), and the inner task runs the shared-trunk launches of csrc/ef_general.hip (DESIGN.md section
    4.12): the trunk runs forward once, and its gradient comes back as one vector, already summed over the nets."""

    def __init__(self, task, beta):
        from .nn import _chain_layers
        m = task.model
        self.task, self.K = task, m.num_reg
        self.enc = _chain_layers(m.encoder)
        self.regs = [_chain_layers(r) for r in m.reg]
        Le, Lr = len(self.enc), len(self.regs[0])
        act0 = self.regs[0][0][1] if Lr >= 2 else 0
        ok = act0 != 0 and [a for _, a in self.enc] == [act0] * (Le - 1) + [0] and all(
            len(r) == Lr and [a for _, a in r] == [act0] * (Lr - 1) + [0] and r[-1][0].out_features == 1 for r in self.regs)
        if not ok or Lr < 2:
            raise NotImplementedError("generator-mode regulariser on MI355X: encoder and regulariser nets must be Linear + activation "
                                      "chains (one activation) ending in a Linear layer, the regulariser nets with at least one hidden layer")
        d_r = self.enc[0][0].in_features
        hidden = [lin.out_features for lin, _ in self.enc[:-1]] + [lin.out_features for lin, _ in self.regs[0][:-1]]
        for r in self.regs:
            assert [lin.out_features for lin, _ in r] == [lin.out_features for lin, _ in self.regs[0]], "regulariser nets differ in shape"
        from .nn import ACT_SIGMOID, ACT_SOFTPLUS
        widths = [w for w in _hip.ef_widths(len(hidden)) if w >= max(hidden)] if 1 <= len(hidden) <= 5 else []
        why = None
        if not widths or self.K > _hip.MAX_NETS:
            why = (f"generator-mode regulariser on MI355X: the chain regulariser o encoder has hidden widths {hidden}; the eigenfunction "
                   f"kernels take 1 to 5 hidden layers of at most {max(_hip.EF_HIDDEN_WIDTHS)} units and at most {_hip.MAX_NETS} nets "
                   "(use lag_tau_reg > 0 - the transfer operator - for other shapes)")
        elif act0 in (ACT_SIGMOID, ACT_SOFTPLUS) and any(h != widths[0] for h in hidden):   # (zero padding needs act(0) = 0)
            why = (f"generator-mode regulariser on MI355X with Sigmoid / Softplus: every hidden width of the chain "
                   f"{hidden} must be one kernel width (no zero padding)")
        # general_nets: a chain without a padded layout runs unpadded, its trunk stored once, on the shared-trunk launches
        self.shared = why is not None and bool(task.general_nets)
        if why is not None and not self.shared:
            raise NotImplementedError(why + ". Pass general_nets=True to RegAutoEncoderTask to run the chain on the shared-trunk "
                                      "kernels of csrc/ef_general.hip.")
        self.H = H = None if self.shared else widths[0]
        self.pdims = [d_r] + (hidden if self.shared else [H] * len(hidden)) + [1]
        act_module = next(mod for mod in m.reg[0]._modules.values() if not isinstance(mod, torch.nn.Linear))
        shared_trunk = None
        if self.shared:   # (the inner task keeps the parameters in a _SharedTrunkFlat: the model only states the architecture)
            shared_trunk = dict(dims=self.pdims, acts=[act0] * len(hidden) + [0], n_shared=Le - 1)
            with torch.device("meta"):
                model = EigenFunctions(self.pdims, self.K, copy.deepcopy(act_module))
        else:
            with torch.random.fork_rng(devices=[]):   # (the virtual nets' initial values are overwritten: leave the caller's RNG stream alone)
                model = EigenFunctions(self.pdims, self.K, copy.deepcopy(act_module))
        tok = np.zeros((4,) + tuple(task._traj_host.shape[1:]), dtype=np.float32)

        class _Tok:
            trajectory, weights, dt, n_frames = tok, np.ones(4), task.traj_dt, 4

        if isinstance(task.preprocessing_layer, AlignFeatureLayer):   # (a frame the alignment accepts: the reference itself)
            _Tok.trajectory = np.zeros_like(tok) + np.random.RandomState(0).normal(size=tok.shape[1:]).astype(np.float32)
        elif task._foreign_pp:   # (frames the module is defined on: the trajectory's own)
            _Tok.trajectory = np.asarray(task._traj_host[np.arange(4) % len(task._traj_host)], dtype=np.float32)
        g0, g1 = float(task.gamma[0]), float(task.gamma[1])
        import tempfile
        # (its own scratch log directory: a second SummaryWriter must not open event files in the user's model_path)
        self._logdir = tempfile.mkdtemp(prefix="cvf_reg_generator_")
        try:
            self.inner = EigenFunctionTask(_Tok, task.preprocessing_layer, model, self._logdir, g1 / g0, [float(v) for v in task._eig_w],
                                           diag_coeff=None, beta=beta, lag_tau=0, learning_rate=task.learning_rate, k=self.K,
                                           batch_size=task.batch_size, device=task.device, verbose=False, save_model_every_step=0,
                                           _shared_trunk=shared_trunk)
        except NotImplementedError as exc:
            if not self.shared:
                raise
            raise NotImplementedError(f"generator-mode regulariser on MI355X (general_nets=True), chain widths {self.pdims}: {exc}") from None
        try:   # nothing is ever logged or stepped through the inner task: close its writer, drop the directory
            close = getattr(self.inner.writer, "close", None)
            if close is not None:
                close()
            import shutil
            shutil.rmtree(self._logdir, ignore_errors=True)
        except Exception:
            pass
        self.n = self.inner._flat.n

    def _params(self):
        ps = [p for lin, _ in self.enc for p in (lin.weight, lin.bias)]
        for r in self.regs:
            ps += [p for lin, _ in r for p in (lin.weight, lin.bias)]
        return ps

    def _theta(self):
        """The virtual parameters as a (differentiable) function of the module's: flat, in the inner model's order."""
        pd, out = self.pdims, []
        We, be = self.enc[-1][0].weight, self.enc[-1][0].bias
        if self.shared:   # the trunk once, then per net the merged layer and the regulariser's remaining layers (_SharedTrunkFlat)
            out = [t for lin, _ in self.enc[:-1] for t in (lin.weight.reshape(-1), lin.bias)]
            for r in self.regs:
                out += [(r[0][0].weight @ We).reshape(-1), r[0][0].weight @ be + r[0][0].bias]
                out += [t for lin, _ in r[1:] for t in (lin.weight.reshape(-1), lin.bias)]
            return torch.cat(out)
        for i in range(self.K):
            r = self.regs[i]
            layers = [(lin.weight, lin.bias) for lin, _ in self.enc[:-1]]
            layers.append((r[0][0].weight @ We, r[0][0].weight @ be + r[0][0].bias))
            layers += [(lin.weight, lin.bias) for lin, _ in r[1:]]
            for l, (W, b) in enumerate(layers):
                fo, fi = pd[l + 1], pd[l]
                out.append(torch.nn.functional.pad(W, (0, fi - W.shape[1], 0, fo - W.shape[0])).reshape(-1))
                out.append(torch.nn.functional.pad(b, (0, fo - b.shape[0])))
        return torch.cat(out)

    def forward(self, X, w, with_grad, dp=False):
        """Loss terms of the batch ``X`` (raw coordinates on the device): returns the inner task's device loss vector
        ``[npl + (gamma_1/gamma_0) pen, npl, pen, eig_1..K sorted, cvec]`` (fp64).  ``dp``: ``X`` is this rank's slice of a global
        batch - the inner task adds its batch sums across the ranks (collective #1) and leaves its gradient local; else the
        batch is evaluated on the calling rank alone."""
        inner = self.inner
        inner._local_only, inner._grad_local = not dp, True
        with torch.enable_grad() if with_grad else torch.no_grad():
            self._tv = self._theta()
        inner._flat.theta.copy_(self._tv.detach())
        inner._flat.repack()
        self._ws = inner._forward(X, w)
        return self._ws.loss_out

    def backward(self, w, scale):
        """Adds ``scale`` * d(npl + (gamma_1/gamma_0) pen)/d(parameter) to the module parameters' slices of the flat gradient."""
        inner, task = self.inner, self.task
        inner._backward(self._ws, w, advance=False, fuse_adam=False)
        views = {id(p): gv for p, _, gv in task._flat.views}
        ps = [p for p in self._params() if not (task.freeze_encoder and any(p is q for lin, _ in self.enc for q in (lin.weight, lin.bias)))]
        grads = torch.autograd.grad(self._tv, ps, grad_outputs=inner._flat.grad * scale, allow_unused=True)
        for p, g in zip(ps, grads):
            if g is not None:
                views[id(p)].add_(g)


class RegAutoEncoderTask(TrainingTask):
    """Regularised autoencoder (arguments, defaults and attributes as core.py:792-816).

    Built on the MI355X path: the time-lagged reconstruction loss (``alpha``, ``lag_tau_ae``, core.py:883-885) and the
    transfer-operator eigenfunction regulariser (``gamma``, ``lag_tau_reg > 0``, core.py:973-1036) - the configurations
    of the reference's notebooks (2d.ipynb:743-760, main.ipynb:452-458) - with ``freeze_encoder``, the variance /
    covariance penalties on the latent vector (``eta[1]``, ``eta[2]``, core.py:912-971) and the gradient-norm penalty of the
    encoder (``eta[0]``, core.py:887-910: :class:`_EncGradPenalty`, on the eigenfunction task's kernels) and the
    regulariser in generator mode (``lag_tau_reg = 0``, core.py:990,1008-1022: :class:`_RegGenerator`, an inner
    :class:`EigenFunctionTask` over the chains regulariser o encoder).

    A step is three launches + the reduction: ``cvf_regae_forward`` (one chain: encoder, then decoder and regulariser
    nets side by side; y on the batch's frames and on their lagged partners, reconstruction error), ``cvf_ef_stats``
    (batch sums, loss tail, d loss / d sum - the eigenfunction task's own kernel), ``cvf_regae_backward`` (forward
    again, output gradients, parameter gradient on the matrix cores, fixed-order reduction, Adam).  A merged chain whose
    parameters and activations do not fit that kernel's 160 KiB of LDS runs the same three calls layer by layer instead
    (``cvf_regae_general_*``: widths up to 4096 units, the same outputs); a chain past both routes is refused with
    NotImplementedError at construction.  Decoder and regulariser nets may have different numbers of layers (nn.py:137-154
    builds the chains independently; the K nets share one ``reg_layer_dims``): that chain (:class:`_RegRaggedFlatParams`) always
    runs layer by layer (``cvf_regae_ragged_*``), with every option.

    ``general_nets`` (not in the reference; default False): the two parts that run on the eigenfunction task's kernels - the
    generator-mode regulariser and ``eta[0]`` - take shapes without a kernel instance too (chains regulariser o encoder and
    encoders of 1 to 11 hidden layers of up to 4096 units, any of the six activations), on the shared-trunk launches of
    csrc/ef_general.hip.  Shapes with an instance keep it, bit for bit; without the option other
    shapes raise NotImplementedError at construction, as before.
    """

    def __init__(self, traj_obj, pp_layer, model, model_path, eig_weights=[], learning_rate=0.01, load_model_filename=None,
                 save_model_every_step=10, batch_size=1000, num_epochs=10, test_ratio=0.2, optimizer_name='Adam', alpha=1.0,
                 gamma=[0.0, 0.0], eta=[0.0, 0.0, 0.0], lag_tau_ae=0, lag_tau_reg=0, beta=1.0, device=torch.device('cuda'),
                 plot_class=None, plot_frequency=0, freeze_encoder=False, verbose=True, debug_mode=True, general_nets=False):
        super().__init__(traj_obj, pp_layer, model, model_path, learning_rate, load_model_filename, save_model_every_step,
                         model.encoded_dim, batch_size, num_epochs, test_ratio, optimizer_name, device, plot_class,
                         plot_frequency, verbose, debug_mode)
        assert isinstance(model, RegAutoEncoder), 'model must be an object of the class RegAutoEncoder'
        assert model.num_reg == len(eig_weights), 'number of weights does not match the number of eigenfunctions!'
        self.alpha, self.gamma, self.eta = alpha, gamma, eta
        self.num_reg = model.num_reg
        self._eps = 1e-5
        self._eig_w = eig_weights
        self._cvec = None
        self.freeze_encoder = freeze_encoder
        # general_nets: the generator-mode regulariser and eta[0] on shapes without a kernel instance run the shared-trunk launches
        # of csrc/ef_general.hip (shapes WITH an instance keep it: the option changes nothing for them), as EigenFunctionTask's
        self.general_nets = bool(general_nets)
        self.traj_dt = traj_obj.dt
        lag_ae_idx, lag_idx = lag_tau_ae / self.traj_dt, lag_tau_reg / self.traj_dt
        assert abs(lag_ae_idx - int(lag_ae_idx)) < 1e-6 and abs(lag_idx - int(lag_idx)) < 1e-6, \
            f'lag-times ({lag_tau_ae}, {lag_tau_reg}) not divisable by the timestep {self.traj_dt} of the trajectory'
        self.lag_ae_idx, self.lag_idx = int(lag_ae_idx), int(lag_idx)
        self._use_reg = self.gamma[0] + self.gamma[1] > self._eps
        if self._use_reg:
            assert self.num_reg > 0, 'number of eigenfunctions must be positive!'
            if self.gamma[0] <= self._eps:
                raise NotImplementedError("RegAutoEncoderTask on MI355X: gamma[0] must be positive when gamma[1] is")
            self._beta = beta
        self._use_enc = max(self.eta[1], self.eta[2]) > self._eps
        # Data-parallel job (one process per GPU): the batch's frames are split over the ranks, the three kinds of batch sums
        # (reconstruction error, latent statistics, regulariser heads) and the gradient are summed across them;
        # the feature trajectory itself is small (d_r floats per frame) and stays whole on every rank.  The two parts that run on
        # an inner EigenFunctionTask (generator-mode regulariser, gradient-norm penalty eta[0]) add their batch sums across the
        # ranks too and leave their gradient shares in the flat gradient, which is summed once, at the end of the step.
        self.init_model_and_optimizer()
        self._n_enc_layers = len([m for m in self.model.encoder if isinstance(m, torch.nn.Linear)])
        # the chain goes per layer (cvf_regae_general_*): decided once, where cvf_regae_route refuses it
        self._general = self._needs_general()
        # --- data: the feature trajectory r(x) of every frame, once (the layer has no parameters), resident in HBM
        traj = _HostFrames(traj_obj.trajectory).all()
        self.tot_dim = int(np.prod(traj.shape[1:]))
        self._weights = torch.as_tensor(np.asarray(traj_obj.weights)).to(device=self.device, dtype=torch.float32).contiguous()
        # pp_layer may be any torch module (core.py:65,122,635): its feature trajectory is computed once with torch
        self._foreign_pp = not isinstance(self.preprocessing_layer, (torch.nn.Identity, AlignFeatureLayer))
        if self.eta[0] > self._eps and not getattr(self.preprocessing_layer, "aligned", True):
            raise NotImplementedError("RegAutoEncoderTask on MI355X: the gradient-norm penalty eta[0] is not built for a feature layer "
                                      "without alignment (PreprocessingANN(None, feature_layer), CVF_PP_FEATURES): its reshape "
                                      "(core.py:907) wants the aligned coordinates as features")
        if self._foreign_pp:
            if _dist.world() > 1:
                raise NotImplementedError("RegAutoEncoderTask with a preprocessing module other than Identity / AlignFeatureLayer "
                                          "runs in single-process jobs only")
            if self.eta[0] > self._eps:
                raise NotImplementedError("RegAutoEncoderTask on MI355X: the gradient-norm penalty eta[0] needs features = coordinates "
                                          "(Identity or AlignFeatureLayer), not a foreign preprocessing module")
            self._pp = self._probe_pp(traj[:1])
        else:
            self._pp = self._pp_desc(self.tot_dim)
        self._feature_traj = self._features(traj)
        d = self._flat.desc
        d_out = self.model.decoder[-1].out_features if self._depths else d.dims[d.n_layers] - self.num_reg
        assert self._pp.d_r == d.dims[0] and d_out == d.dims[0], 'encoder input / decoder output width must equal the feature dimension'
        if self.verbose:
            print('\nShape of trajectory data array:\n {}'.format(tuple(traj.shape)), flush=True)
        cfg = _hip.EFCfg()
        K = max(self.num_reg, 1)
        cfg.k, cfg.lag_idx, cfg.sort_eigvals = K, max(self.lag_idx, 1), 1          # cvec = argsort always (core.py:1016)
        cfg.alpha = float(self.gamma[1] / self.gamma[0]) if self._use_reg else 0.0  # gamma_0 (npl + gamma_1/gamma_0 pen)
        cfg.beta, cfg.dt = float(beta), float(self.traj_dt)
        for i in range(self.num_reg):
            cfg.eig_w[i] = float(eig_weights[i])
        self._cfg = cfg
        ecfg = _hip.EFCfg()                      # batch sums of the latent vector (the generator-mode layout, E unused)
        ecfg.k, ecfg.lag_idx, ecfg.sort_eigvals, ecfg.alpha, ecfg.beta, ecfg.dt = self.k, 0, 0, 0.0, 1.0, 1.0
        self._ecfg = ecfg
        self._ws = {}
        self._enc_grad = _EncGradPenalty(self) if self.eta[0] > self._eps else None   # (raises here when the encoder does not fit)
        # generator-mode regulariser (lag_tau_reg = 0): needs the coordinates themselves (its derivative runs through r(x))
        self._traj_host = traj
        self._gen = _RegGenerator(self, beta) if self._use_reg and self.lag_idx == 0 else None
        # (with a foreign module the inner task takes its records [r | L] instead: pp.FactoredMetric, CVF_PP_FACTORED)
        self._traj = None if self._gen is None else self._gen.inner._frames(traj)

    # -- the base class builds the flat buffer from mlp_layout(); this model needs the side-by-side chain
    #    (decoder and regulariser nets of different depths: the ragged one, cvf_regae_ragged_*)
    def _flat_params(self):
        from .nn import _chain_layers
        depths = {len(_chain_layers(net)) for net in [self.model.decoder] + (list(self.model.reg) if self.model.num_reg > 0 else [])}
        flat = (_RegFlatParams if len(depths) == 1 else _RegRaggedFlatParams)(self.model, self.device, self.freeze_encoder)
        # (n_dec_layers, n_reg_layers) behind n_enc_layers in every cvf_regae_ragged_* call; () on the equal-depth routes
        self._depths = (flat.n_dec, flat.n_reg) if isinstance(flat, _RegRaggedFlatParams) else ()
        return flat

    def _needs_general(self):
        """False where the fused chain kernel takes the merged chain (cvf_regae_route: a 64-frame tile's chain in LDS), True where
        only the per-layer route of csrc/regae_general.hip does - then for every pass, loss-only ones included; a chain past both
        is refused here, at construction.  (The layout with a gradient is the larger one: where it fits, the forward pass does.)"""
        lib, fl = _hip.lib(), self._flat
        if self._depths:   # different depths always go per layer (the fused kernel runs the two groups layer for layer)
            if lib.cvf_regae_ragged_supported(fl.desc, self.num_reg, self._n_enc_layers, *self._depths) != 1:
                raise NotImplementedError("RegAutoEncoderTask: no HIP route trains this chain (%s)" % lib.cvf_last_error().decode())
            return True
        if lib.cvf_regae_route(fl.desc, 1, None) >= 0:
            return False
        fused = lib.cvf_last_error().decode()
        if lib.cvf_regae_general_supported(fl.desc, self.num_reg, self._n_enc_layers) != 1:
            raise NotImplementedError("RegAutoEncoderTask: no HIP route trains this chain (%s; %s)"
                                      % (fused, lib.cvf_last_error().decode()))
        return True

    def colvar_model(self):
        """core.py:855-863."""
        return _CVModel(self.preprocessing_layer, self.model.encoder, device=self.device)

    def reg_model(self):
        """core.py:865-877."""
        if self._cvec is None:
            self._cvec = torch.arange(self.model.num_reg)
        return _CVModel(self.preprocessing_layer, RegModel(self.model, self._cvec), device=self.device)

    def _workspace(self, B):
        ws = self._ws.get(B)
        if ws is None:
            lib, K, dev = _hip.lib(), max(self.num_reg, 1), self.device
            T = _hip.ntiles(B)
            if self._depths:
                size = lib.cvf_regae_ragged_scratch_floats(self._flat.desc, B, self.num_reg, self._n_enc_layers, *self._depths)
            else:
                size = (lib.cvf_regae_general_scratch_floats if self._general else lib.cvf_regae_scratch_floats)(self._flat.desc, B)
            ws = dict(
                scratch=torch.empty(size, device=dev, dtype=torch.float32),
                y=torch.zeros(2 * T * K * 64, device=dev, dtype=torch.float32),
                out2=torch.zeros(3, device=dev, dtype=torch.float64),
                stats=torch.zeros(lib.cvf_ef_nstats(K, 1), device=dev, dtype=torch.float64),
                sscratch=torch.zeros(lib.cvf_ef_stats_scratch_doubles(K, 1), device=dev, dtype=torch.float64),
                loss_vec=torch.zeros(3 + 2 * K, device=dev, dtype=torch.float64),
                coef=torch.zeros(4 * K + K * K, device=dev, dtype=torch.float64), T=T)
            # (small) latent-vector buffers: the public reg_enc_* functions need them whatever eta is
            k = self.k
            ws.update(enc=torch.zeros(T * k * 64, device=dev, dtype=torch.float32),
                      ezero=torch.zeros(T * k * 64, device=dev, dtype=torch.float32),
                      estats=torch.zeros(lib.cvf_ef_nstats(k, 0), device=dev, dtype=torch.float64),
                      esscratch=torch.zeros(lib.cvf_ef_stats_scratch_doubles(k, 0), device=dev, dtype=torch.float64),
                      eterms=torch.zeros(2, device=dev, dtype=torch.float64),
                      ecoef=torch.zeros(k + k * k, device=dev, dtype=torch.float64))
            self._ws[B] = ws
        return ws

    def _step(self, feat, idx, w, w_lag, lag_ae, lag_reg, with_grad, advance=False, wsum=None, out=None, X=None, dp=False):
        """Loss terms (and, with ``with_grad``, gradient + optimizer step) of one batch: rows ``idx`` of ``feat``
        (``None``: rows 0..B-1), targets at ``+lag_ae``, lagged partners at ``+lag_reg``.  ``wsum``: the batch's weight
        sum when the caller knows it (static batches), else one host read.  Returns (or fills ``out`` with) the device
        vector [loss, ae, npl, pen, eig_1..K, enc_grad, enc_norm, enc_orth] (fp64).  ``X``: the batch's raw coordinates for the
        generator-mode regulariser (``None``: rows ``idx`` of the resident trajectory).  ``dp``: the batch is this rank's slice of a
        global batch (``train()`` of a data-parallel job) - batch sums and gradient are summed across the ranks; the public loss
        functions below evaluate the batch they are handed, on the calling rank alone."""
        lib, fl, P = _hip.lib(), self._flat, _hip.ptr
        B, K = int(w.shape[0]), self.num_reg
        ws = self._workspace(B)
        use_reg = self._use_reg and K > 0
        gen = self._gen if use_reg and lag_reg == 0 else None    # generator mode: the regulariser runs on the eigenfunction task's kernels
        assert not (use_reg and lag_reg == 0 and gen is None), 'generator-mode regulariser needs gamma and lag_tau_reg = 0 at construction'
        use_reg = use_reg and gen is None     # (from here on: the transfer-operator regulariser inside the chain kernels)
        alpha = float(self.alpha) if self.alpha > self._eps else 0.0
        use_enc = self._use_enc
        eta1 = float(self.eta[1]) if self.eta[1] > self._eps else 0.0
        eta2 = float(self.eta[2]) if self.eta[2] > self._eps else 0.0
        # (with a gradient to follow, the statistics pass leaves its activations in the scratch buffer for the gradient pass)
        if self._depths:
            fwd = fwd_keep = lib.cvf_regae_ragged_forward
            bwd_reuse = lib.cvf_regae_ragged_backward_reuse
        elif self._general:
            fwd = fwd_keep = lib.cvf_regae_general_forward
            bwd_reuse = lib.cvf_regae_general_backward_reuse
        else:
            fwd, fwd_keep, bwd_reuse = lib.cvf_regae_forward, lib.cvf_regae_forward_keep, lib.cvf_regae_backward_reuse
        self._call("cvf_regae_forward", fwd_keep if with_grad else fwd, fl.desc, P(fl.theta),
                   P(feat), P(idx), B, lag_ae, lag_reg if use_reg else 0, K, P(w), P(ws["scratch"]), P(ws["y"]), self._n_enc_layers,
                   *self._depths, P(ws["enc"]) if use_enc else None, P(ws["out2"]), _hip.stream())
        if dp:
            self._allreduce("allreduce_batch_sums", ws["out2"])     # [sum w err, sum w, (ratio: recomputed by cvf_regae_loss_row)]
        if use_enc:   # core.py:912-971: weighted means / variances / covariances of the latent vector, then the two penalties
            self._call("cvf_ef_stats", lib.cvf_ef_stats, self._ecfg, B, P(w), P(ws["enc"]), P(ws["ezero"]), None, None,
                       P(ws["esscratch"]), P(ws["estats"]), None, None, _hip.stream())
            if dp:
                self._allreduce("allreduce_batch_sums", ws["estats"])
            self._call("cvf_regae_enc_loss", lib.cvf_regae_enc_loss, P(ws["estats"]), self.k, eta1, eta2, P(ws["eterms"]),
                       P(ws["ecoef"]), _hip.stream())
        if use_reg:
            y_lag = ws["y"][ws["T"] * K * 64:]
            self._call("cvf_ef_stats", lib.cvf_ef_stats, self._cfg, B, P(w), P(ws["y"]), None, P(w_lag), P(y_lag),
                       P(ws["sscratch"]), P(ws["stats"]), None if dp else P(ws["loss_vec"]), None if dp else P(ws["coef"]), _hip.stream())
            if dp:
                self._allreduce("allreduce_batch_sums", ws["stats"])
                self._call("cvf_ef_loss", lib.cvf_ef_loss, self._cfg, P(ws["stats"]), P(ws["loss_vec"]), P(ws["coef"]), _hip.stream())
            self._cvec_dev = ws["loss_vec"][3 + K:3 + 2 * K]
        if out is None:
            out = torch.zeros(7 + K, device=self.device, dtype=torch.float64)
        self._call("cvf_regae_loss_row", lib.cvf_regae_loss_row, P(ws["out2"]), P(ws["loss_vec"]) if use_reg else None, alpha,
                   float(self.gamma[0]) if use_reg else 0.0, float(self.gamma[1]) if use_reg else 0.0, K,
                   P(ws["eterms"]) if use_enc else None, eta1, eta2, P(out), _hip.stream())
        eg = self._enc_grad if self.eta[0] > self._eps else None
        rows = None
        if eg is not None:   # core.py:1092-1095: the gradient-norm penalty of the encoder, on the eigenfunction kernels
            rows = feat[:B] if idx is None else feat.index_select(0, idx)
        if with_grad:
            if wsum is None:
                wsum_t = w.sum(dtype=torch.float64)
                if dp:
                    _dist.allreduce_sum_(wsum_t)
                wsum = float(wsum_t)
            adam = self.optimizer.fused_args() if advance and eg is None and gen is None and not dp else None   # (their gradients are added before the update)
            self._call("cvf_regae_backward", bwd_reuse, fl.desc, P(fl.theta), P(feat), P(idx), B, lag_ae,
                       lag_reg if use_reg else 0, K, P(w), P(w_lag) if use_reg else None, alpha / wsum,
                       float(self.gamma[0]) if use_reg else 0.0, P(ws["y"]) if use_reg else None,
                       P(ws["coef"]) if use_reg else None, self._n_enc_layers, *self._depths, P(ws["ecoef"]) if use_enc else None,
                       P(ws["scratch"]), P(fl.grad), P(fl.mask),
                       P(self.optimizer.step_count) if advance else None, adam, _hip.stream())
        if gen is not None:
            lv = gen.forward(X if X is not None else (self._traj[:B] if idx is None else self._traj.index_select(0, idx)), w, with_grad, dp)
            out[2:4] = lv[1:3]
            out[4:4 + K] = lv[3:3 + K]
            out[0] += float(self.gamma[0]) * lv[1] + float(self.gamma[1]) * lv[2]
            self._cvec_dev = lv[3 + K:3 + 2 * K]
            if with_grad:
                gen.backward(w, float(self.gamma[0]))
        if eg is not None:
            term = eg.run(rows, w, float(self.eta[0]), with_grad and not self.freeze_encoder, dp)
            out[4 + K] = term
            out[0] += float(self.eta[0]) * term
        if with_grad and dp:
            self._allreduce("allreduce_gradient", fl.grad)      # collective #2: every part's share, once
        if with_grad and advance and adam is None:
            self.optimizer.step(advance=False)
        return out

    # -- the reference's public loss functions, evaluated on raw coordinate batches (forward values; the training
    #    loop below uses the resident feature trajectory instead)
    def _terms(self, feat, w, w_lag, lag_ae, lag_reg, alpha, use_reg, use_enc):
        """Forward values with only the named parts of the loss switched on."""
        keep = (self.alpha, self._use_reg, self._use_enc, self.eta)
        self.alpha, self._use_reg, self._use_enc, self.eta = alpha, use_reg, use_enc, [0.0, 1.0, 1.0] if use_enc else [0.0, 0.0, 0.0]
        try:
            return self._step(feat, None, w, w_lag, lag_ae, lag_reg, with_grad=False)
        finally:
            self.alpha, self._use_reg, self._use_enc, self.eta = keep

    def weighted_MSE_loss(self, X, X_lagged, weight):
        """core.py:879-885."""
        B = int(torch.as_tensor(X).shape[0])
        feat = torch.cat([self._features(X), self._features(X_lagged)])
        return self._terms(feat, self._dev(weight), None, B, 0, 1.0, False, False)[1].to(torch.get_default_dtype())

    def reg_eigen_loss(self, X, weight, X_lagged, weight_lagged):
        """core.py:973-1036 (transfer operator): ``(eig_vals, non_penalty_loss, penalty, cvec)``."""
        assert self.num_reg > 0, 'needs regularisers'
        if self.lag_idx == 0:   # generator mode (core.py:990,1008-1022): X_lagged / weight_lagged are not used
            assert self._gen is not None, 'generator-mode regulariser needs gamma at construction'
            Xd = self._gen.inner._frames(torch.as_tensor(X).detach())
            lv = self._gen.forward(Xd, self._dev(weight), False)
            dt, K = torch.get_default_dtype(), self.num_reg
            return lv[3:3 + K].to(dt).cpu(), lv[1].to(dt), lv[2].to(dt), lv[3 + K:3 + 2 * K].cpu().to(torch.long).numpy()
        B = int(torch.as_tensor(X).shape[0])
        feat = torch.cat([self._features(X), self._features(X_lagged)])
        gam, self.gamma = self.gamma, (self.gamma if self._use_reg else [1.0, 1.0])
        try:
            out = self._terms(feat, self._dev(weight), self._dev(weight_lagged), 0, B, 0.0, True, False)
        finally:
            self.gamma = gam
        dt = torch.get_default_dtype()
        cvec = self._cvec_dev.cpu().to(torch.long).numpy()
        return out[4:4 + self.num_reg].to(dt).cpu(), out[2].to(dt), out[3].to(dt), cvec

    def reg_enc_grad_loss(self, X, weight):
        """core.py:887-910 (forward value)."""
        if self._foreign_pp:
            raise NotImplementedError("reg_enc_grad_loss needs features = coordinates (Identity or AlignFeatureLayer)")
        if self._enc_grad is None:
            self._enc_grad = _EncGradPenalty(self)
        return self._enc_grad.run(self._features(X), self._dev(weight), 1.0, False).to(torch.get_default_dtype())

    def _enc_terms(self, X, weight):
        out = self._terms(self._features(X), self._dev(weight), None, 0, 0, 0.0, False, True)
        return out[5 + self.num_reg:].to(torch.get_default_dtype())

    def reg_enc_norm_loss(self, X, weight):
        """core.py:912-934."""
        return self._enc_terms(X, weight)[0]

    def reg_enc_orthognal_loss(self, X, weight):
        """core.py:936-971."""
        return self._enc_terms(X, weight)[1]

    def train(self):
        """core.py:1038-1217."""
        ll = self._feature_traj.shape[0] - max(self.lag_idx, self.lag_ae_idx)           # core.py:1042
        idx_train, idx_test = _agreed_split(ll, self.test_ratio, 1, self.device)         # core.py:1044 (one draw)
        bs_train, bs_test = min(self.batch_size, len(idx_train)), min(self.batch_size, len(idx_test))
        world = _dist.world()

        def resident(idx, bs):
            """(rows of the feature trajectory, weights, lagged weights, batches) of the permuted set `idx` for this process: a
            data-parallel job keeps this rank's contiguous slice of every static batch (_static_batches)."""
            pos, _, bl = _static_batches(len(idx), bs)
            it = torch.as_tensor(np.asarray(idx)[pos], device=self.device, dtype=torch.long)
            return it, self._weights[it].contiguous(), self._weights[it + self.lag_idx].contiguous(), bl

        itr, wtr, wtr_lag, tr_batches = resident(idx_train, bs_train)
        ite, wte, wte_lag, te_batches = resident(idx_test, bs_test)
        wsum_tr = _batch_weight_sums(wtr, tr_batches)
        self.loss_list = []
        min_loss = float("inf")
        self._announce((bs_train, bs_test), (len(itr) * world, len(ite) * world), (len(tr_batches), len(te_batches)))
        K = self.num_reg
        loss_names = ['loss', 'ae_loss', 'eigen_non_penalty', 'eigen_penalty'] + ['eig_%d' % i for i in range(K)] + \
                     ['encoder_gradient', 'encoder_norm', 'encoder_orthogonality']
        log_tr, log_te = self._epoch_logs(len(tr_batches), len(te_batches), len(loss_names))
        cvec_log = [torch.zeros(max(K, 1), dtype=torch.float64).pin_memory() for _ in range(4)]   # the ordering, with the ring below

        def on_epoch(ep, tr, te):
            dt = torch.get_default_dtype()
            tr, te = tr.to(dt), te.to(dt)
            if self._use_reg and (tr_batches or te_batches):
                self._cvec = cvec_log[ep % len(cvec_log)][:K].clone().to(torch.long)          # core.py:1110 (last evaluation)
            self.loss_list.append([tr, te])                                                       # core.py:1202
            self._write_epoch_means(loss_names, ep, tr, te)                                       # core.py:1208-1212

        elog = _AsyncEpochLog(log_tr, log_te, len(tr_batches), len(te_batches), on_epoch)
        dp = _dist.collectives()
        for epoch in _tqdm(range(self.num_epochs), disable=(_dist.rank() != 0)):
            self.model.train()
            for it, (a, b) in enumerate(tr_batches):
                self._step(self._feature_traj, itr[a:b], wtr[a:b], wtr_lag[a:b], self.lag_ae_idx, self.lag_idx, with_grad=True,
                           advance=True, wsum=wsum_tr[it], out=log_tr[it], dp=dp)
            saving, plotting = self._due(epoch)
            if saving or plotting:                       # (order of the reference: save / plot before the test pass, core.py:1130-1140)
                if self._use_reg and tr_batches:
                    self._cvec = self._cvec_dev.cpu().to(torch.long)
            if saving:
                last = float(log_tr[len(tr_batches) - 1, 0]) if tr_batches else float("inf")
                min_loss = self._save_latest_and_best(epoch, last, min_loss)
            if plotting:
                self._plot(epoch)
            for it, (a, b) in enumerate(te_batches):
                self._step(self._feature_traj, ite[a:b], wte[a:b], wte_lag[a:b], self.lag_ae_idx, self.lag_idx, with_grad=False,
                           out=log_te[it], dp=dp)
            elog.reserve(epoch)
            if self._use_reg and (tr_batches or te_batches):
                cvec_log[epoch % len(cvec_log)].copy_(self._cvec_dev, non_blocking=True)
            elog.push(epoch)
        elog.flush_all()
        self._loss_frames(loss_names)
