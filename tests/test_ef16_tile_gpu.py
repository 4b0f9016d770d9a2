"""GPU (-m gpu): the feature tile of a resident batch (csrc/ef16_front_rows.hip, EigenFunctionTask._alignment_rows).

The features of the 16-frame step - aligned positions - depend on the frames and the layer only, so the launch that fills a
resident batch's alignment rows writes its feature tile too, and the hot front launch reads that tile instead of rebuilding it.
The bar is BIT FOR BIT (torch.equal): fill kernel and solving front kernel evaluate the same device function on the same
records, so there is no arithmetic difference to grant a tolerance for.

* the tile of the fill launch equals the tile cvf_ef16_front writes, padding columns included, and the rows of the new entry
  equal those of cvf_ef16_align_rows - at B = 69 (two tiles: four whole units, a ragged one, three of padding only) over the
  16-byte copy path of the stager, the general stager with a prefix of align atoms, d_r = 72 (S = SMAX and the clamp edge), and
  coordinates that are not features;
* a hot step neither writes nor rebuilds a tile: the entry's tile is unchanged and the workspace's own feature buffers,
  NaN-filled before the first step, are still NaN after three steps (so the backward launch read the cached tile);
* an in-place write to the frames refills rows and tile in place, and the step equals the uncached task's.
"""

import gc

import pytest
import torch

from tests import ef_cases as E
from tests.synth import make_molecule_traj
from tests.test_ef16_rows_gpu import CASE, _entries, _pair, _same, _step, _task

pytestmark = pytest.mark.gpu

B69 = 69
#        id                         (n_atoms, n_rec, n_align)  hidden        k
LAYERS = [("copy-path-nit6", (22, 22, 22), (20, 20, 20), 3),   # 16-byte copy path of the stager, NIT 6
          ("general-prefix", (7, 7, 5), (12, 12), 2),          # general stager, ALLAL false
          ("dr72-clamp-edge", (24, 24, 24), (16,), 2),         # d_r = 72: S = SMAX and the clamp edge
          ("coords-not-features", (5, 3, 3), (8, 8, 8), 1)]    # coordinates that are not features


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _collect_tasks():
    yield
    gc.collect()
    torch.cuda.synchronize()


@pytest.mark.parametrize("name,layer,hidden,k", LAYERS, ids=[l[0] for l in LAYERS])
def test_fill_tile_equals_front_tile(dev, monkeypatch, name, layer, hidden, k):
    from colvarsfinder import _hip
    n_atoms, n_rec, n_align = layer
    case = E.Case(name, "gen", n_atoms, n_rec, n_align, "pos", hidden, k, B69, False, False)
    assert E.route(case) == "ef16"
    traj, w, ref = make_molecule_traj(n_atoms, B69, seed=9100 + n_atoms, scale=2.0, sigma=0.3)
    task = _task(dev, monkeypatch, False, n_atoms, n_rec, n_align, hidden, k, ref, traj[:64], w[:64])
    X = torch.tensor(traj, dtype=torch.float32, device=dev).reshape(B69, -1).contiguous()
    wt = torch.tensor(w, dtype=torch.float32, device=dev)
    lib, P = _hip.lib(), _hip.ptr
    ws = task._workspace(B69)
    for t in ws._feat:
        t.fill_(float("nan"))
    task._events = {}
    task.loss_func(X, wt, None, None)   # cvf_ef16_front: solves, and writes the tile into the workspace
    assert "cvf_ef16_front" in task._events and not _entries(task)
    task._events = None
    front_tile = ws.feat.clone()
    d_r, T = 3 * n_rec, E.n_tiles(B69)
    assert front_tile.numel() == T * d_r * E.TILE and torch.isfinite(front_tile).all()   # every column of 4 T units is written

    n_rows = int(lib.cvf_ef16_align_rows_floats(B69))
    assert n_rows == 4 * T * E.UNIT * E.AUX_PITCH + 4
    rows_old = torch.full((n_rows,), float("nan"), device=dev)
    rows_new = torch.full((n_rows,), float("nan"), device=dev)
    tile = torch.full((T * d_r * E.TILE,), float("nan"), device=dev)
    _hip.check(lib.cvf_ef16_align_rows(task._pp, P(X), B69, P(rows_old), _hip.stream()), "cvf_ef16_align_rows")
    _hip.check(lib.cvf_ef16_align_rows_tile(task._pp, P(X), B69, P(rows_new), P(tile), _hip.stream()), "cvf_ef16_align_rows_tile")
    torch.cuda.synchronize()
    assert torch.equal(rows_new, rows_old), int((rows_new != rows_old).sum())
    assert torch.equal(tile, front_tile), int((tile != front_tile).sum())
    # frames past B replicate the last one: columns 5..63 of the second tile repeat column 4
    last, n_last = tile.reshape(T, d_r, E.TILE)[1], B69 - E.TILE
    assert torch.equal(last[:, n_last:], last[:, n_last - 1:n_last].expand(-1, E.TILE - n_last))


def test_hot_step_leaves_the_tile_alone(dev, monkeypatch):
    (tc, Xc, wc), _ = _pair(dev, monkeypatch, CASE)
    ws = tc._workspace(CASE.B)
    for t in ws._feat:
        t.fill_(float("nan"))
    assert _step(tc, Xc, wc)[3] == 1
    (ent,) = _entries(tc)
    tile = ent[3]
    first = tile.clone()
    assert torch.isfinite(first).all()
    for _ in range(2):
        assert _step(tc, Xc, wc)[3] == 0
    assert torch.equal(tile, first)
    assert all(torch.isnan(t).all() for t in ws._feat)   # no tile written or rebuilt; the backward launch read the entry's
    d_r = 3 * CASE.n_rec
    assert tile.numel() == ws.Tt * d_r * E.TILE and tc.feature_tile_bytes == 4 * ws.Tt * d_r * E.TILE
    assert tc.alignment_rows_bytes == 4 * (4 * E.n_tiles(CASE.B) * E.UNIT * E.AUX_PITCH + 4) == 4 * ent[2].numel()
    tc.drop_alignment_cache()
    assert tc.feature_tile_bytes == 0 and tc.alignment_rows_bytes == 0


def test_inplace_write_refills_rows_and_tile(dev, monkeypatch):
    (tc, Xc, wc), (tu, Xu, wu) = _pair(dev, monkeypatch, CASE)
    _same(_step(tc, Xc, wc), _step(tu, Xu, wu), "before the write")
    (ent,) = _entries(tc)
    rows, tile = ent[2], ent[3]
    rows_before, tile_before = rows.clone(), tile.clone()
    for X in (Xc, Xu):
        X.add_(0.25 * torch.sin(torch.arange(X.numel(), device=dev, dtype=torch.float32)).reshape(X.shape))
    c, u = _step(tc, Xc, wc), _step(tu, Xu, wu)
    assert c[3] == 1, c[3]   # one launch refills both
    _same(c, u, "after the write")
    (ent,) = _entries(tc)
    assert ent[2] is rows and ent[3] is tile   # in place: a captured graph may hold the addresses
    assert not torch.equal(tile, tile_before) and not torch.equal(rows, rows_before)
    _same(_step(tc, Xc, wc), _step(tu, Xu, wu), "hot again")
