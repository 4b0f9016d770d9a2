"""Network containers with the module/parameter layout of the reference's ``colvarsfinder.nn``.

API twin of reference ``colvarsfinder/nn.py`` (own code): same class names, constructor
arguments, attribute names and ``state_dict`` keys, so models, checkpoints and user scripts
are interchangeable:

* ``create_sequential_nn`` (nn.py:29-59): ``Linear`` children named ``'1'..'L'``, the
  activation (ONE shared instance) registered as ``'activation i'`` after every layer but
  the last.
* ``EigenFunctions`` (nn.py:242-293), ``AutoEncoder`` (nn.py:61-114),
  ``RegAutoEncoder`` (nn.py:116-203), ``RegModel`` (nn.py:205-239).

These classes are parameter containers plus a plain ``forward`` (used for inference and
TorchScript export).  Training on the MI355X never calls ``forward``: the tasks in
``colvarsfinder.core`` flatten the parameters into one HBM buffer and run the hand-written
HIP kernels on it (``mlp_layout`` below describes that buffer to the C ABI).
"""

import re

import numpy as np
import torch


def create_sequential_nn(layer_dims, activation=torch.nn.Tanh()):
    """Feed-forward net ``layer_dims[0] -> ... -> layer_dims[-1]`` (activation between layers only)."""
    n = len(layer_dims)
    assert n >= 2, f"Error: at least 2 layers are needed to define a neural network (length={n})!"
    net = torch.nn.Sequential()
    for pos, (d_in, d_out) in enumerate(zip(layer_dims[:-1], layer_dims[1:]), start=1):
        net.add_module(str(pos), torch.nn.Linear(d_in, d_out))
        if pos < n - 1:
            net.add_module(f"activation {pos}", activation)
    return net


def _encoder_cv_params(encoder, n_encoder_layers, cv_idx):
    """Named parameters of an encoder restricted to output ``cv_idx`` (last layer sliced to one row)."""
    picked = []
    for name, param in encoder.named_parameters():
        layer = int(re.search(r"\d+", name).group())
        picked.append([name, param if layer < n_encoder_layers else param[cv_idx:cv_idx + 1, ...]])
    return picked


class AutoEncoder(torch.nn.Module):
    """``encoder`` / ``decoder`` pair; ``forward(x) = decoder(encoder(x))``."""

    def __init__(self, e_layer_dims, d_layer_dims, activation=torch.nn.Tanh()):
        super().__init__()
        assert e_layer_dims[-1] == d_layer_dims[0], "ouput dimension of encoder and input dimension of decoder do not match!"
        self.encoder = create_sequential_nn(e_layer_dims, activation)
        self.decoder = create_sequential_nn(d_layer_dims, activation)
        self.encoded_dim = e_layer_dims[-1]
        self._num_encoder_layer = len(e_layer_dims) - 1

    def get_params_of_cv(self, cv_idx):
        assert 0 <= cv_idx < self.encoded_dim, f"index {cv_idx} exceeded the range [0, {self.encoded_dim-1}]!"
        return _encoder_cv_params(self.encoder, self._num_encoder_layer, cv_idx)

    def forward(self, inp):
        return self.decoder(self.encoder(inp))


class RegAutoEncoder(torch.nn.Module):
    """Autoencoder plus ``K`` scalar regulariser nets on the latent space."""

    def __init__(self, e_layer_dims, d_layer_dims, reg_layer_dims, K, activation=torch.nn.Tanh()):
        super().__init__()
        assert e_layer_dims[-1] == d_layer_dims[0], "ouput dimension of encoder and input dimension of decoder do not match!"
        self.num_reg = K
        assert K == 0 or e_layer_dims[-1] == reg_layer_dims[0], \
            "ouput dimension of encoder and input dimension of regulator part do not match!"
        self.encoder = create_sequential_nn(e_layer_dims, activation)
        self.decoder = create_sequential_nn(d_layer_dims, activation)
        self.encoded_dim = e_layer_dims[-1]
        self._num_encoder_layer = len(e_layer_dims) - 1
        self.reg = torch.nn.ModuleList(create_sequential_nn(reg_layer_dims, activation) for _ in range(K)) if K > 0 else None

    def get_params_of_cv(self, cv_idx):
        assert 0 <= cv_idx < self.encoded_dim, f"index {cv_idx} exceeded the range [0, {self.encoded_dim-1}]!"
        return _encoder_cv_params(self.encoder, self._num_encoder_layer, cv_idx)

    def forward_ae(self, inp):
        return self.decoder(self.encoder(inp))

    def forward_reg(self, inp):
        assert self.num_reg > 0, "number of regularizers is not positive."
        z = self.encoder(inp)
        return torch.cat([net(z) for net in self.reg], dim=1)

    def forward(self, inp):
        z = self.encoder(inp)
        return torch.cat((self.decoder(z), torch.cat([net(z) for net in self.reg], dim=1)), dim=1)


class RegModel(torch.nn.Module):
    """Regulariser nets of a :class:`RegAutoEncoder` evaluated in the order ``cvec``."""

    def __init__(self, reg_ae, cvec):
        super().__init__()
        assert reg_ae.num_reg > 0, "number of regularizers is not positive."
        assert len(cvec) == reg_ae.num_reg, "length of cvec doesn't equal to number of regularizers"
        assert (sorted(cvec) == np.arange(reg_ae.num_reg)).all(), f"cvec should be a permutation of 0,1,...,{len(cvec)-1}."
        self.encoder = reg_ae.encoder
        self.reg = reg_ae.reg
        self.cvec = cvec
        self.encoded_dim = reg_ae.encoded_dim
        self.num_reg = reg_ae.num_reg

    def forward(self, inp):
        z = self.encoder(inp)
        return torch.cat([self.reg[idx](z) for idx in self.cvec], dim=1)


class EigenFunctions(torch.nn.Module):
    """``k`` scalar nets of identical architecture; ``forward`` concatenates their outputs to ``[l, k]``."""

    def __init__(self, layer_dims, k, activation=torch.nn.Tanh()):
        super().__init__()
        assert layer_dims[-1] == 1, "each eigenfunction must be scalar-valued"
        self.eigen_funcs = torch.nn.ModuleList(create_sequential_nn(layer_dims, activation) for _ in range(k))

    def get_params_of_cv(self, cv_idx):
        return [[name, param] for name, param in self.eigen_funcs[cv_idx].named_parameters()]

    def forward(self, inp):
        return torch.cat([net(inp) for net in self.eigen_funcs], dim=1)


class SharedEigenFunctions(EigenFunctions):
    """``k`` scalar eigenfunctions on ONE trunk (the VAMPnets / SRV form ``[d_r, H, .., H, k]``; not in the reference).

    ``trunk_dims = [d_r, h_1, .., h_m]``, ``m >= 1``: Linear layers shared by all ``k`` eigenfunctions, each followed by
    ``activation``.  ``head_dims = [h_m, .., 1]``, at least one Linear layer: ``k`` independent copies, ``activation`` between
    their layers and none after the last.  ``head_dims = [h_m, 1]`` is the classic multi-output net.

    ``eigen_funcs[i]`` is the chain trunk -> head ``i`` as a ``create_sequential_nn``-shaped ``Sequential`` whose first ``m``
    Linear layers are the SAME module objects for every ``i``: ``parameters()`` yields every trunk tensor once (trunk, head 0,
    head 1, ..), ``state_dict()`` names it under every ``eigen_funcs.i`` (the keys of an ``EigenFunctions`` of the full chain),
    a deep copy keeps the sharing, and ``get_params_of_cv(i)`` returns the trunk's and head ``i``'s parameters.
    ``n_shared = m`` is what the kernels are told (csrc/ef_general.hip: cvf_ef_general_shared_*)."""

    def __init__(self, trunk_dims, head_dims, k, activation=torch.nn.Tanh()):
        torch.nn.Module.__init__(self)
        trunk_dims, head_dims = list(trunk_dims), list(head_dims)
        assert len(trunk_dims) >= 2, "the trunk needs at least one Linear layer"
        assert len(head_dims) >= 2, "a head needs at least one Linear layer"
        assert head_dims[0] == trunk_dims[-1], "output dimension of the trunk and input dimension of the heads do not match!"
        assert head_dims[-1] == 1, "each eigenfunction must be scalar-valued"
        assert k >= 1, "at least one eigenfunction is needed"
        self.n_shared = m = len(trunk_dims) - 1
        trunk = [torch.nn.Linear(a, b) for a, b in zip(trunk_dims[:-1], trunk_dims[1:])]
        n = m + len(head_dims) - 1
        nets = []
        for _ in range(k):
            net = torch.nn.Sequential()
            head = [torch.nn.Linear(a, b) for a, b in zip(head_dims[:-1], head_dims[1:])]
            for pos, lin in enumerate(trunk + head, start=1):
                net.add_module(str(pos), lin)
                if pos < n:
                    net.add_module(f"activation {pos}", activation)
            nets.append(net)
        self.eigen_funcs = torch.nn.ModuleList(nets)


# ----------------------------------------------------------------------------------------------
# Flat-buffer description of a model for the HIP kernels (not part of the reference API)
# ----------------------------------------------------------------------------------------------

# activation codes of include/cvf.h (cvf_mlp_desc.act); 1 == True, so "followed by Tanh" still reads as a flag
ACT_NONE, ACT_TANH, ACT_SIGMOID, ACT_RELU, ACT_ELU, ACT_LEAKY_RELU, ACT_SOFTPLUS = range(7)


def _act_code(module):
    """cvf_mlp_desc.act code of a torch activation module (the reference takes any, nn.py:29-59); the chain kernels of the
    autoencoder tasks implement these, with the modules' default parameters."""
    if isinstance(module, torch.nn.Tanh):
        return ACT_TANH
    if isinstance(module, torch.nn.Sigmoid):
        return ACT_SIGMOID
    if isinstance(module, torch.nn.ReLU):
        return ACT_RELU
    if isinstance(module, torch.nn.ELU) and module.alpha == 1.0:
        return ACT_ELU
    if isinstance(module, torch.nn.LeakyReLU) and module.negative_slope == 0.01:
        return ACT_LEAKY_RELU
    if isinstance(module, torch.nn.Softplus) and module.beta == 1.0 and module.threshold == 20.0:
        return ACT_SOFTPLUS
    raise NotImplementedError(
        f"the MI355X kernels implement Tanh, Sigmoid, ReLU, ELU(alpha=1), LeakyReLU(0.01) and Softplus(beta=1, threshold=20) "
        f"(got {module})")


def _chain_layers(seq):
    """[(Linear, activation code that follows it - 0: none)] of a create_sequential_nn module; rejects anything else."""
    out = []
    children = list(seq._modules.values())  # children() would drop the repeats of the shared activation
    for i, child in enumerate(children):
        if isinstance(child, torch.nn.Linear):
            nxt = children[i + 1] if i + 1 < len(children) else None
            has_act = nxt is not None and not isinstance(nxt, torch.nn.Linear)
            out.append((child, _act_code(nxt) if has_act else ACT_NONE))
    return out


def _strict_chain_layers(seq):
    """``_chain_layers`` for a module nobody vouches for: the same list when ``seq`` is a plain ``Sequential`` of ``Linear`` layers
    (with bias, widths that chain), each followed by at most one activation the kernels implement - what ``create_sequential_nn``
    builds.  TypeError (with the reason) for anything else."""
    if type(seq) is not torch.nn.Sequential:
        raise TypeError(f"{type(seq).__name__} is not a create_sequential_nn chain")
    children, out, i = list(seq._modules.values()), [], 0
    while i < len(children):
        lin, act = children[i], ACT_NONE
        if type(lin) is not torch.nn.Linear or lin.bias is None:
            raise TypeError(f"child {i} of the chain ({type(lin).__name__}) is not a Linear layer with a bias")
        if out and out[-1][0].out_features != lin.in_features:
            raise TypeError(f"child {i} of the chain takes {lin.in_features} inputs, the layer before it has {out[-1][0].out_features} outputs")
        if i + 1 < len(children) and not isinstance(children[i + 1], torch.nn.Linear):
            try:
                act = _act_code(children[i + 1])
            except NotImplementedError:
                raise TypeError(f"no HIP kernel for the activation {children[i + 1]}") from None
            i += 1
        out.append((lin, act))
        i += 1
    if not out:
        raise TypeError("the chain has no Linear layer")
    return out


def mlp_layout(model):
    """Describe ``model`` as chains of Linear layers over ONE flat fp32 buffer laid out in
    ``model.parameters()`` order.  Returns dict(nets=[[(w_off, b_off, in, out, act), ...], ...], n_params).
    ``EigenFunctions``, ``AutoEncoder``, or a bare ``create_sequential_nn`` chain such as an encoder (checked strictly: TypeError
    when the module is anything else)."""
    offsets, pos = {}, 0
    for p in model.parameters():
        offsets[id(p)] = pos
        pos += p.numel()
    if isinstance(model, EigenFunctions):
        chains = [_chain_layers(net) for net in model.eigen_funcs]
        # (the eigenfunction kernels need the activation's first two derivatives: the 16-frame kernels carry tanh's, the
        #  64-frame kernels take every code above - csrc/ef_mfma.hip: ef_shape; other shapes are rejected by the task)
    elif isinstance(model, AutoEncoder):
        chains = [_chain_layers(model.encoder) + _chain_layers(model.decoder)]
    elif type(model) is torch.nn.Sequential:
        chains = [_strict_chain_layers(model)]
    else:
        raise TypeError(f"no HIP layout for model type {type(model).__name__}")
    nets = [[(offsets[id(lin.weight)], offsets[id(lin.bias)], lin.in_features, lin.out_features, int(act))
             for lin, act in chain] for chain in chains]
    return dict(nets=nets, n_params=pos)
