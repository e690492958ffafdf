"""The frame resize on the device (-m gpu): tmpnn_frames_resize against Pillow's recorded output (tests/golden/resize) and the
host definition resize_host / prep_host, byte for byte and bit for bit, in both output forms; FramePrep.prep; and
FrameStore.from_raw against its host-only twin."""
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'resize')
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
# (h, w) -> (H, W): up on both axes, 3 taps | down on both, 7 taps, odd W | up vertically, 15 taps horizontally | horizontal pass
# only | vertical pass only | copy | bounds clamped at both ends | about 87 taps
CASES = ['37x61_to_48x80', '50x70_to_20x33', '23x45_to_33x7', '9x9_to_9x17', '9x17_to_5x17', '64x64_to_64x64', '3x2_to_11x5',
         '5x300_to_1x7']
SENT = 0xA5


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import __graft_entry__
    __graft_entry__.build()


@pytest.fixture(scope='module')
def table():
    from trackmpnn_amd.frames import norm_table
    return norm_table(MEAN, STD)[2]


def _resize(src: np.ndarray, HW, table=None, shift: int = 0):
    """tmpnn_frames_resize of src [n, h, w, 3] into a window of a sentinel-filled buffer (`shift` elements past a 16-byte
    boundary): (the output [n, 3, H, W] on the host, True when every byte around the window kept its sentinel)."""
    from trackmpnn_amd.frames import _DeviceResize
    dev = torch.device(DEV)
    n, (H, W) = src.shape[0], HW
    numel, pad = n * 3 * H * W, 64
    size = 4 if table is not None else 1
    raw = torch.full(((numel + 2 * pad) * size,), SENT, dtype=torch.uint8, device=dev)
    buf = raw.view(torch.float32) if table is not None else raw
    out = buf[pad + shift:pad + shift + numel].view(n, 3, H, W)
    assert out.data_ptr() % 16 == (shift * size) % 16
    table_d = None if table is None else torch.from_numpy(table).to(dev)
    _DeviceResize(HW, dev).run(torch.from_numpy(src).to(dev), out, table_d)
    got = out.cpu().numpy()
    edges = raw.cpu().numpy()
    lo, hi = (pad + shift) * size, (pad + shift + numel) * size
    return got, bool((edges[:lo] == SENT).all() and (edges[hi:] == SENT).all())


@pytest.mark.parametrize('shift', [0, 1])
@pytest.mark.parametrize('name', CASES)
def test_device_equals_pillow_and_the_host_definition(name, shift, table):
    """n = 3 frames in one call (random bytes, all 255 -- the accumulator's top --, columns alternating 0 / 255): the uint8 form
    equals Pillow's recorded bytes and resize_host; the float32 form equals prep_host bit for bit; nothing is written outside the
    output, whether it starts on a 16-byte boundary (vector stores where W allows) or one element behind (single stores)."""
    from trackmpnn_amd import prep_host, resize_host
    d = np.load(os.path.join(GOLDEN, name + '.npz'))
    src, want = d['src'], d['out']
    assert src.shape[0] == 3 and (src[1] == 255).all()
    HW = want.shape[1:3]
    got, clean = _resize(src, HW, None, shift)
    assert clean
    assert np.array_equal(got, want.transpose(0, 3, 1, 2)), name
    assert np.array_equal(got, resize_host(src, HW).transpose(0, 3, 1, 2))
    gotf, clean = _resize(src, HW, table, shift)
    assert clean
    assert np.array_equal(gotf.view(np.uint32), prep_host(src, HW, table).view(np.uint32)), name
    # one frame alone: the same bytes as its slice of the batch
    one, _ = _resize(src[2:3], HW, None, shift)
    assert np.array_equal(one[0], got[2])


def test_every_fixture_is_a_case():
    assert sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, '*.npz'))) == sorted(CASES)


def test_a_kitti_frame_equals_the_host_definition(table):
    """375 x 1242 -> 384 x 1280: many workgroups, 16-byte loads and stores on every row, in both forms."""
    from trackmpnn_amd import prep_host, resize_host
    src = np.random.default_rng(7).integers(0, 256, (1, 375, 1242, 3), dtype=np.uint8)
    want = resize_host(src, (384, 1280))
    got, clean = _resize(src, (384, 1280))
    assert clean and np.array_equal(got, want.transpose(0, 3, 1, 2))
    gotf, clean = _resize(src, (384, 1280), table)
    assert clean and np.array_equal(gotf.view(np.uint32), prep_host(src, (384, 1280), table).view(np.uint32))


def test_frame_prep_equals_prep_host(table):
    """A host array, a host tensor and a device tensor, one frame and a batch, two source sizes through one FramePrep (its
    coefficient tables are cached per source size)."""
    from trackmpnn_amd import FramePrep, prep_host
    prep = FramePrep((48, 80), MEAN, STD, device=DEV)
    assert np.array_equal(prep.table.view(np.uint32), table.view(np.uint32))
    rng = np.random.default_rng(11)
    a = rng.integers(0, 256, (37, 61, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (2, 50, 70, 3), dtype=np.uint8)
    for frame, src in ((a, a), (torch.from_numpy(a), a), (torch.from_numpy(a).to(DEV), a), (b, b), (torch.from_numpy(b).to(DEV), b),
                       (a, a)):
        got = prep.prep(frame)
        want = prep_host(src, (48, 80), table)
        assert got.device.type == 'cuda' and got.dtype == torch.float32 and tuple(got.shape) == want.shape
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert sorted(prep._rs._tables) == [(37, 61), (50, 70)]


def test_from_raw_on_the_device_equals_its_host_twin(monkeypatch):
    """Two sequences of different sizes, resized on the device two frames a call: gather(plan) of the device store equals
    frames_host(plan) of the host-only store bit for bit, mirrored rows included."""
    from trackmpnn_amd import FrameStore, frames
    monkeypatch.setattr(frames, 'RESIZE_BATCH', 2)
    rng = np.random.default_rng(5)
    raw = [rng.integers(0, 256, (3, 37, 61, 3), dtype=np.uint8), rng.integers(0, 256, (5, 23, 45, 3), dtype=np.uint8)]
    for hw in ((48, 80), (20, 33)):
        dev = FrameStore.from_raw(raw, hw, MEAN, STD, device=DEV)
        host = FrameStore.from_raw(raw, hw, MEAN, STD, device=None)
        assert np.array_equal(dev.raw_hw, [[37, 61], [23, 45]]) and np.array_equal(dev.raw_hw, host.raw_hw)
        assert np.array_equal(dev.planar_d.cpu().numpy(), host.planar)
        plan = np.array([[s, f, m] for s in (0, 1) for f in range(raw[s].shape[0]) for m in (0, 1)])
        got = dev.gather(plan).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), host.frames_host(plan).view(np.uint32))
        assert np.array_equal(got.view(np.uint32), dev.frames_host(plan).view(np.uint32))
