"""CPU: what the 16-frame backward launch (csrc/ef16_back.hip) got back when its uniform values left the wave's path,
read as tests/test_kernel_resources.py reads it - from the metadata of the code objects `make` built (the numbers are those of
-Rpass-analysis=kernel-resource-usage) - and the host's refusal of a net layout the kernel has no offsets for.

On the parent commit every instance spilled between 53 and 168 scalar registers into lanes of vector registers (the benchmark's
`<20, 3, false, true>`: 142, in three vector registers of 127), because the body of the tile loop is some eighty uniform row
offsets that the compiler computed in front of the loop.  The one-tile form is now straight-line code and spills nothing; the
multi-tile form keeps the loop with D, k and the lane opaque inside it.

PARENT: (VGPRs, scratch bytes per lane, SGPR spills) of every instance on the parent commit.  The bars are "no more than measured
on this tree", capped at the parent's value: they can only ratchet down.
"""
import os

import pytest

from tests.codeobj import built_objects, kernels_of, template_args

# (H, NH, MULTI, GEN) -> (vgpr_count, private_segment_fixed_size, sgpr_spill_count) on the parent commit
PARENT = {
    (8, 1, 0, 0): (70, 0, 84), (8, 1, 0, 1): (80, 0, 53), (8, 1, 1, 0): (70, 0, 86), (8, 1, 1, 1): (80, 0, 59),
    (8, 2, 0, 0): (82, 0, 96), (8, 2, 0, 1): (104, 0, 72), (8, 2, 1, 0): (82, 0, 97), (8, 2, 1, 1): (96, 0, 75),
    (8, 3, 0, 0): (80, 0, 100), (8, 3, 0, 1): (103, 0, 76), (8, 3, 1, 0): (80, 0, 102), (8, 3, 1, 1): (94, 0, 79),
    (12, 1, 0, 0): (70, 0, 86), (12, 1, 0, 1): (85, 0, 63), (12, 1, 1, 0): (72, 0, 88), (12, 1, 1, 1): (87, 0, 65),
    (12, 2, 0, 0): (88, 0, 100), (12, 2, 0, 1): (104, 0, 77), (12, 2, 1, 0): (89, 0, 103), (12, 2, 1, 1): (104, 0, 81),
    (12, 3, 0, 0): (86, 0, 103), (12, 3, 0, 1): (102, 0, 86), (12, 3, 1, 0): (88, 0, 105), (12, 3, 1, 1): (104, 0, 90),
    (16, 1, 0, 0): (70, 0, 90), (16, 1, 0, 1): (92, 0, 65), (16, 1, 1, 0): (70, 0, 91), (16, 1, 1, 1): (93, 0, 68),
    (16, 2, 0, 0): (87, 0, 111), (16, 2, 0, 1): (114, 0, 84), (16, 2, 1, 0): (78, 0, 103), (16, 2, 1, 1): (106, 0, 87),
    (16, 3, 0, 0): (85, 0, 110), (16, 3, 0, 1): (116, 0, 92), (16, 3, 1, 0): (86, 0, 110), (16, 3, 1, 1): (106, 0, 95),
    (20, 1, 0, 0): (87, 0, 101), (20, 1, 0, 1): (100, 0, 80), (20, 1, 1, 0): (88, 0, 103), (20, 1, 1, 1): (102, 0, 82),
    (20, 2, 0, 0): (101, 0, 131), (20, 2, 0, 1): (126, 0, 115), (20, 2, 1, 0): (95, 0, 140), (20, 2, 1, 1): (126, 0, 123),
    (20, 3, 0, 0): (101, 0, 149), (20, 3, 0, 1): (127, 0, 142), (20, 3, 1, 0): (99, 0, 150), (20, 3, 1, 1): (128, 0, 148),
    (24, 2, 0, 0): (88, 0, 122), (24, 2, 0, 1): (125, 0, 111), (24, 2, 1, 0): (89, 0, 130), (24, 2, 1, 1): (125, 0, 113),
    (24, 3, 0, 0): (89, 0, 134), (24, 3, 0, 1): (128, 44, 135), (24, 3, 1, 0): (89, 0, 142), (24, 3, 1, 1): (128, 40, 139),
    (32, 2, 0, 0): (119, 0, 134), (32, 2, 0, 1): (128, 68, 149), (32, 2, 1, 0): (95, 0, 138), (32, 2, 1, 1): (128, 80, 130),
    (32, 3, 0, 0): (117, 0, 152), (32, 3, 0, 1): (128, 200, 168), (32, 3, 1, 0): (99, 0, 153), (32, 3, 1, 1): (128, 212, 160),
}
# the four H = 20, NH = 3 instances as measured on this tree: (VGPRs, SGPR spills)
MEASURED = {(20, 3, 0, 0): (78, 0), (20, 3, 0, 1): (111, 0), (20, 3, 1, 0): (91, 55), (20, 3, 1, 1): (119, 44)}


@pytest.fixture(scope="module")
def back(tmp_path_factory):
    ks = kernels_of(os.path.join(built_objects(), "ef16_back.o"), tmp_path_factory.mktemp("ef16_back"))
    out = {template_args(n, "ef16_back_kernel"): v for n, v in ks.items() if template_args(n, "ef16_back_kernel") is not None}
    assert set(out) == set(PARENT), "the instance list is the parent's: 16 (H, NH) x MULTI x GEN"
    return out


def test_benchmark_instance_got_its_registers_back(back):
    v = back[(20, 3, 0, 1)]
    assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0, v
    assert v["vgpr_count"] < 127 and v["sgpr_spill_count"] < 142, v
    for key, (vgprs, spills) in MEASURED.items():
        v = back[key]
        assert vgprs <= PARENT[key][0] and spills <= PARENT[key][2]
        assert v["vgpr_count"] <= vgprs and v["sgpr_spill_count"] <= spills, (key, v)
        assert v.get("private_segment_fixed_size", 0) == 0 and v.get("vgpr_spill_count", 0) == 0, (key, v)


def test_no_instance_takes_more_than_on_the_parent(back):
    for key, (vgprs, scratch, spills) in PARENT.items():
        v = back[key]
        assert v["vgpr_count"] <= vgprs, (key, v)
        assert v.get("private_segment_fixed_size", 0) <= scratch, (key, v)
        assert v["sgpr_spill_count"] <= spills, (key, v)


def test_one_tile_form_spills_no_scalar_register(back):
    """Straight-line code: nothing is computed in front of a loop and carried through lanes of a vector register."""
    for key, v in back.items():
        if key[2] == 0:
            assert v["sgpr_spill_count"] == 0, (key, v)


# ------------------------------------------------------------------------------------------------ the host's side of the record
def _desc(H, dims, k, edit=None):
    d = H.MLPDesc()
    d.n_nets, d.n_layers = k, len(dims) - 1
    pos = 0
    for i in range(k):
        for l in range(len(dims) - 1):
            d.dims[l], d.dims[l + 1], d.act[l] = dims[l], dims[l + 1], int(l + 2 < len(dims))
            d.w_off[i][l], d.b_off[i][l] = pos, pos + dims[l] * dims[l + 1]
            pos += (dims[l] + 1) * dims[l + 1]
    d.n_params = pos
    if edit is not None:
        edit(d)
    return d


def _swap_hidden_layers(d):
    """Layers 1 and 2 of net 1 change places inside the net's span (same sizes: both are 20 x 20 + 20)."""
    d.w_off[1][1], d.w_off[1][2] = d.w_off[1][2], d.w_off[1][1]
    d.b_off[1][1], d.b_off[1][2] = d.b_off[1][2], d.b_off[1][1]


def _bias_first(d):
    """Layer 1 of net 0 keeps its place but stores the bias in front of the weight."""
    d.b_off[0][1] = d.w_off[0][1]
    d.w_off[0][1] = d.b_off[0][1] + 20


def _bias_displaced(d):
    """The bias of layer 1 of net 0 does not start where the weight ends."""
    d.b_off[0][1] += 1


@pytest.mark.parametrize("edit,why", [(_swap_hidden_layers, "net 1: layer 1 does not follow layer 0"), (_bias_first, "net 0: layer 1 does not follow layer 0"),
                                      (_bias_displaced, "net 0, layer 1: the bias does not follow the weight")])
def test_a_layout_the_kernel_has_no_offsets_for_is_refused_before_any_launch(edit, why):
    """No GPU here: the call returns its negative code without touching the device (the buffers are never read).  The kernel derives a
    layer's offsets from its net's base; a permuted net passes the older contiguity checks and would be written to the wrong rows."""
    import __graft_entry__  # noqa: F401  (puts the package on sys.path)
    from colvarsfinder import _hip as H
    built_objects()
    lib = H.lib()
    cfg = H.EFCfg()
    cfg.k, cfg.lag_idx = 2, 0
    fake = 4096   # a non-null address that is never dereferenced
    d = _desc(H, [66, 20, 20, 20, 1], 2, edit)
    assert lib.cvf_ef16_backward(cfg, d, fake, fake, 87, fake, fake, fake, fake, fake, fake, None, fake, None) < 0
    assert why in lib.cvf_last_error().decode(), lib.cvf_last_error()
    cfg.lag_idx = 2
    assert lib.cvf_ef16_backward_transfer(cfg, d, fake, fake, 87, fake, fake, fake, fake, fake, fake, None, fake, None) < 0
    assert why in lib.cvf_last_error().decode(), lib.cvf_last_error()
