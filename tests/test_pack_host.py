"""CPU (-m "not gpu"): where the fragment scatter of csrc/cvf_pack.hpp puts every parameter.  pack_tab_fill + pack_scatter - the
source that cvf_ef_pack and every optimiser kernel inline - are compiled in hipcc's HOST pass into the stand-alone program
tools/pack_host.hip (AddressSanitizer + UBSan: a slot outside the buffer ends the run) which scatters parameter p with the
value p + 1 into a zeroed fragment buffer.  For every (H, NH) the eigenfunction kernels are instantiated for
(optim_cases.EF_SHAPES), D = 1..136 and a few wide first layers, and 1, 3 and 8 nets:

  - every weight of the layers in front of the output layer sits on exactly two slots, both inside its own net's range: one in
    the layer's forward region (F0 / Fh_l) and one in its transposed region (T0 / Th_l), the regions being the ones the layout
    comment of cvf_pack.hpp states: per net [F0: S1*RT][Fh_l: NG*RT][Th_l: NG*RT][T0: CT*NG] fragments of 64 floats;
  - biases and the output layer land nowhere, every other slot is 0.

No two parameters share a slot: the program scatters the parameters in ascending and in descending order and counts the slots
that differ between the two - a slot with two writers keeps the later one, so it would differ.  (Two slots per weight, none for
the rest and zeros elsewhere say the same once more: a shared slot would leave one of its parameters on fewer than two.)"""
import os
import subprocess

import numpy as np
import pytest

from tests import optim_cases as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def pack_host(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("pack") / "pack_host")
    subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "--cuda-host-only", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "colvars-finder_amd", "csrc"), os.path.join(ROOT, "tools", "pack_host.hip"), "-o", out],
                   check=True, timeout=300)

    def run(cases):
        text = "".join("%d %d %d %d\n" % c for c in cases)
        r = subprocess.run([out], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        return r.stdout

    return run


def test_shapes_are_the_compiled_instances():
    """A width added to the kernels' dispatch (colvarsfinder._hip.ef_widths) must be added to optim_cases.EF_SHAPES."""
    import __graft_entry__  # noqa: F401  (puts the package on sys.path)
    from colvarsfinder import _hip
    shapes = [(h, nh) for nh in range(1, 6) for h in _hip.ef_widths(nh)]
    assert len(shapes) == 24 and sorted(shapes) == sorted(OC.EF_SHAPES)
    assert _hip.ef_widths(6) == ()


def regions(H, NH, D):
    """(per_net, {layer: ((F begin, F end), (T begin, T end))}) in floats, from the layout comment of csrc/cvf_pack.hpp."""
    NG = (H + 3) // 4
    RT = (NG + 3) // 4
    S1, CT = (D + 3) // 4, (D + 15) // 16
    sizes = [S1 * RT] + [NG * RT] * (NH - 1) + [NG * RT] * (NH - 1) + [CT * NG]
    starts = np.concatenate([[0], np.cumsum(sizes)]) * 64
    reg = {0: ((starts[0], starts[1]), (starts[2 * NH - 1], starts[2 * NH]))}
    for l in range(1, NH):
        reg[l] = ((starts[l], starts[l + 1]), (starts[NH - 1 + l], starts[NH + l]))
    return int(starts[-1]), reg


def check_case(H, NH, D, k, per_net_got, n_params_got, buf):
    per_net, reg = regions(H, NH, D)
    dims = [D] + [H] * NH + [1]
    per_net_params = sum(dims[l + 1] * (dims[l] + 1) for l in range(NH + 1))
    tag = (H, NH, D, k)
    assert per_net_got == per_net and n_params_got == k * per_net_params, tag
    assert buf.size == k * per_net, tag
    val = buf.astype(np.int64)
    assert np.array_equal(val.astype(np.float32), buf), tag          # whole numbers only
    slots = np.flatnonzero(val)
    prm = val[slots] - 1
    assert prm.min() >= 0 and prm.max() < n_params_got, tag
    count = np.bincount(prm, minlength=n_params_got)
    # which layer every parameter is a weight of (-1: a bias or the output layer)
    layer = np.full(n_params_got, -1)
    pos = 0
    for n in range(k):
        for l in range(NH + 1):
            nw = dims[l + 1] * dims[l]
            if l < NH:
                layer[pos:pos + nw] = l
            pos += nw + dims[l + 1]
    assert np.array_equal(count, np.where(layer >= 0, 2, 0)), tag
    # (with the counts above: 2 * weights slots are taken, each by one parameter, and the rest of the buffer is 0)
    assert slots.size == 2 * int((layer >= 0).sum()), tag
    order = np.argsort(prm, kind="stable")                           # slots ascend within a parameter
    pair = slots[order].reshape(-1, 2)
    who = prm[order].reshape(-1, 2)[:, 0]
    net = who // per_net_params
    rel = pair - (net * per_net)[:, None]
    assert (rel >= 0).all() and (rel < per_net).all(), tag           # inside its own net's range
    assert (pair[:, 0] != pair[:, 1]).all(), tag
    lay = layer[who]
    for l in range(NH):
        (f0, f1), (t0, t1) = reg[l]
        sel = lay == l
        assert sel.sum() == k * dims[l + 1] * dims[l], tag
        assert ((rel[sel, 0] >= f0) & (rel[sel, 0] < f1)).all(), (tag, l, "forward region")
        assert ((rel[sel, 1] >= t0) & (rel[sel, 1] < t1)).all(), (tag, l, "transposed region")


@pytest.mark.parametrize("H,NH", OC.EF_SHAPES)
def test_every_weight_on_its_two_slots(pack_host, H, NH):
    cases = [(H, NH, D, k) for D in OC.PACK_HOST_D for k in OC.PACK_HOST_NETS]
    out = pack_host(cases)
    pos = 0
    for c in cases:
        head = np.frombuffer(out, np.int32, 7, pos)
        assert tuple(head[:4]) == c
        assert head[6] == 0, (c, "slots with more than one writer", int(head[6]))
        n = c[3] * int(head[4])
        buf = np.frombuffer(out, np.float32, n, pos + 28)
        pos += 28 + 4 * n
        check_case(*c, int(head[4]), int(head[5]), buf)
    assert pos == len(out)


def test_the_check_sees_a_collision_and_a_stray_slot():
    """The checker itself: a buffer with one weight's slot overwritten by its neighbour, and one with a bias scattered, fail."""
    H, NH, D, k = 8, 2, 5, 2
    per_net, reg = regions(H, NH, D)
    per_net_params = H * (D + 1) + H * (H + 1) + H + 1
    buf = np.zeros(k * per_net, np.float32)
    # a valid assignment built by hand: weights of layer l in order over the first slots of its F and T regions
    pos = 0
    for n in range(k):
        for l in range(NH):
            nw = H * (D if l == 0 else H)
            for r in (0, 1):
                b = n * per_net + reg[l][r][0]
                buf[b:b + nw] = np.arange(pos, pos + nw) + 1
            pos += nw + H
        pos += H + 1
    check_case(H, NH, D, k, per_net, k * per_net_params, buf)
    bad = buf.copy()
    bad[0] = bad[1]                                                  # parameter 1 took parameter 0's slot
    with pytest.raises(AssertionError):
        check_case(H, NH, D, k, per_net, k * per_net_params, bad)
    bad = buf.copy()
    bad[reg[0][0][1] - 1] = H * D + 1                                # the first bias landed on a free slot
    with pytest.raises(AssertionError):
        check_case(H, NH, D, k, per_net, k * per_net_params, bad)

