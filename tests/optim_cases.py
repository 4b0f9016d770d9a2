"""Shapes and settings of the optimiser tests (tests/test_pack_host.py on the CPU, tests/test_optimizer_gpu.py on the GPU), in
plain Python: importing this module needs neither torch nor the built library."""

# every (hidden width, hidden layers) the eigenfunction kernels are instantiated for (csrc/ef_mfma.hip: ef_dispatch; tied to
# colvarsfinder._hip.ef_widths by tests/test_pack_host.py::test_shapes_are_the_compiled_instances)
EF_SHAPES = ([(h, nh) for h in (8, 12, 16, 20) for nh in (1, 2, 3)] + [(h, nh) for h in (24, 32, 48, 64) for nh in (2, 3)] +
             [(h, nh) for h in (20, 32) for nh in (4, 5)])

# ---- tests/test_pack_host.py: first-layer widths and net counts per shape
PACK_HOST_D = tuple(range(1, 137)) + (192, 200, 256, 384, 385)
PACK_HOST_NETS = (1, 3, 8)

# ---- slab reduction: both instantiations (<= 64 rows: 4 row groups, more: 32) and the edges of their rounds of 4 x 10 and
# 32 x 10 loads; parameter counts around the 32 parameters of a block
SLAB_ROWS = (1, 2, 3, 4, 5, 39, 40, 41, 64, 65, 319, 320, 321, 1024, 2049)
SLAB_PARAMS = (1, 31, 32, 33, 6603)

# ---- Adam / SGD: sizes around the 256 threads of a block, the flagship parameter count, and one past the 1024 x 256
# threads of the largest grid (grid-stride loop)
OPT_SIZES = (1, 255, 256, 257, 6603, 262144 + 37)
ADAM_STEPS = (1, 2, 10, 1000, 100000)
GRAD_SCALES = (1e-12, 1e-6, 1e-2, 1.0, 1e6, 1e12)
# lr: passed by value; lr_dev: the device scalar that overrides it (None: no device scalar)
ADAM_HYPER = {
    "default": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, lr_dev=None),
    "fast": dict(lr=0.05, betas=(0.8, 0.99), eps=1e-6, lr_dev=None),
    "lr_dev": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, lr_dev=0.0173),
}
SGD_LR = {"value": dict(lr=0.01, lr_dev=None), "lr_dev": dict(lr=0.01, lr_dev=0.37)}
ADAM_BAR_FACTOR, ADAM_BAR_FLOOR = 4.0, 2.0 ** -22

# ---- fragment refresh by every updater: D and the number of nets rotate over the shapes
REFRESH_D = (1, 2, 3, 5, 16, 17, 66, 72, 127, 128, 129, 200)
REFRESH_CASES = [(h, nh, REFRESH_D[i % len(REFRESH_D)], 1 + i % 8) for i, (h, nh) in enumerate(EF_SHAPES)]
REFRESH_UPDATERS = ("adam_step", "slab_adam_5", "slab_adam_70", "sgd_step")

# ---- the full pack at first-layer widths the instance sweeps do not reach: cvf_ef_mlp_fwd (y and g = dy/dfeat) on one full
# and one ragged tile, one narrow and one wide shape per depth; the number of nets rotates
FWD_B = 70
FWD_D = (1, 2, 5, 17, 127, 128, 129, 200)
FWD_SHAPES = ((8, 1), (20, 1), (8, 2), (64, 2), (12, 3), (48, 3), (20, 4), (32, 4), (20, 5), (32, 5))
FWD_CASES = [(h, nh, d, 1 + (i + j) % 3) for i, (h, nh) in enumerate(FWD_SHAPES) for j, d in enumerate(FWD_D)]
# (y, g) bars, each error taken over the largest entry of its case: 8 x the worst distance of the fp32 CPU evaluation with
# pinned roundings (tests/optim_inputs.py: fwd_pinned32) from the fp64 nets of oracle/nnref.py over FWD_CASES, rounded up to
# two digits; tests/test_optim_cases.py holds both between 4 x and 16 x of that figure.
FWD_BARS = (5.5e-6, 7.5e-6)   # worst e32: 6.79e-7 (y), 9.27e-7 (g)
