"""noisediff_amd.diffusion_data: the diffusion model's training and generation batches from resident uint16 Bayer frames, one HIP launch each
(nd_raw_diffusion_batch_f32, csrc/raw.hip).

CPU: the numpy restatement (tests/diffusion_data_ref.py) equals the reference's own dataset code (tests/golden/diffusion_data.npz, captured by
tests/golden/capture_diffusion_data.py) bit for bit; random_params consumes np.random as SonyTrainDataset.aug does; bad arguments are refused
without a GPU; balanced_sample_list and frame_batches restate the reference's lists.
GPU: the launch equals the restatement bit for bit on every uint16 code, on every addressing path and for every subset of outputs; a bad table row
gives NaN for its sample only; the builders equal the goldens, capture into graphs and feed GaussianDiffusion.forward and .sample.  Every
comparison asks for zero difference.  Outputs are pre-filled with NaN and longer than the kernel writes."""
import ctypes as C
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import diffusion_data_ref as D
from noisediff_amd import synth

DEV = torch.device("cuda", 0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAN = float("nan")
KEYS = ("noise", "noisy_img", "clean_img", "coord")              # the entry point's argument order
SUBSETS = [KEYS, ("noise", "clean_img", "coord"), ("clean_img", "coord"), ("coord",)]


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(GOLDEN, "diffusion_data.npz"))
    seed, (H2, W2) = int(z["meta.seed"]), (int(v) for v in z["meta.shape"])
    frames = {n: np.floor(synth.uniform(seed, f"diffusion_data.{n}", (H2, W2), lo, hi).numpy()).astype(np.uint16)
              for n, lo, hi in (("short", 480.0, 700.0), ("long", 400.0, 17500.0))}
    return SimpleNamespace(z=z, seed=seed, frames=frames, H=H2 // 2, W=W2 // 2, crop=int(z["meta.crop"]), n=int(z["meta.n_train"]),
                           pairs=[(int(i), float(r)) for i, r in z["meta.pairs"]], mapping=[int(v) for v in z["meta.mapping"]],
                           patches=[(int(x), int(y)) for x, y in z["meta.patches"]])


# --------------------------------------------------------------------------- CPU 1: the restatement against the reference

def test_restatement_equals_every_golden_array(gold):
    z, f, c = gold.z, gold.frames, gold.crop
    free = []
    for i in range(gold.n):
        x0, y0 = (int(v) for v in z[f"train.{i}.xy"])
        got = D.sample(f["short"], f["long"], x0, y0, c, c, gold.pairs[i % 3][1])
        for key in KEYS:
            assert got[key].dtype == np.float32 and np.array_equal(got[key], z[f"train.{i}.{key}"]), (i, key)
        assert float(got["clean_img"].max()) > 1 and float(got["noise"].min()) < -1           # clean_img is not clipped
        assert 0.02 < float(((got["noisy_img"] > 0) & (got["noisy_img"] < 1)).mean()) and float((got["noisy_img"] == 1).mean()) > 0.02
        assert int(z[f"train.{i}.iso_ratio_idx"]) == gold.mapping[i % 3]
        free.append(len(z[f"train.{i}.randint"]) == 2)
    assert any(free) and not all(free)                                                      # both branches of aug are among the samples
    for j, (x, y) in enumerate(gold.patches):
        got = D.sample(None, f["long"], x, y, c, c, 1.0)
        assert np.array_equal(got["clean_img"], z[f"gen.{j}.clean_img"]) and np.array_equal(got["coord"], z[f"gen.{j}.coord"])
    whole = D.coord(1424, 2128, 0, 0, 1424, 2128)                                           # make_coord at the SID geometry
    assert np.array_equal(whole[0, :, 0], z["sid.coord_rows"]) and np.array_equal(whole[1, 0, :], z["sid.coord_cols"])
    assert whole[0, -1, 0] == 1 and whole[1, 0, -1] == 1 and (whole[0] == whole[0, :, :1]).all() and (whole[1] == whole[1, :1, :]).all()


# --------------------------------------------------------------------------- CPU 2: host logic

def test_random_params_draws_as_the_reference_does(gold):
    from noisediff_amd import diffusion_data as dd
    z, c, H, W = gold.z, gold.crop, gold.H, gold.W
    b = dd.DiffusionBatchBuilder(c)
    state = np.random.get_state()
    try:
        np.random.seed(gold.seed)
        for i in range(gold.n):                               # one sample at a time, in the capture's order: the recorded windows come back
            assert b.random_params(1, (H, W)) == {"xy": [tuple(int(v) for v in z[f"train.{i}.xy"])]}
        after = np.random.randint(1 << 30)
        np.random.seed(gold.seed)
        got = b.random_params(gold.n, (H, W))["xy"]           # and as one batch
        assert np.random.randint(1 << 30) == after
        np.random.seed(gold.seed)
        for i in range(gold.n):                               # the reference's calls, replayed: no draw more and none less
            u = np.random.uniform()
            assert u == float(z[f"train.{i}.uniform"])
            x = np.random.randint(0, W - c + 1)
            y = np.random.randint(0, H - c + 1) if u < 0.5 else H - c - 1
            assert [x] + ([y] if u < 0.5 else []) == z[f"train.{i}.randint"].tolist() and got[i] == (x, y)
            if u >= 0.5:
                assert got[i][1] == H - c - 1                 # the bottom band, one short of the last row
        assert np.random.randint(1 << 30) == after
        b.random_params(2, (c + 1, c))
        with pytest.raises(ValueError):
            b.random_params(1, (c, W))                        # H == crop: the band's y would be -1
        with pytest.raises(ValueError):
            b.random_params(1, (H, c - 1))
    finally:
        np.random.set_state(state)


def test_builders_refuse_bad_parameters_on_the_host():
    from noisediff_amd import _lib as L, diffusion_data as dd, raw
    with pytest.raises(ValueError):
        dd.DiffusionBatchBuilder(crop=0)
    b = dd.DiffusionBatchBuilder(crop=16)
    shape = (2, 64, 96)
    ok = dict(short=[0, 1], long=[1, 0], xy=[(0, 0), (31, 15)], ratio=[100, 250])
    rows = b.check(2, shape, **ok)[32:].view(raw.ROW)
    assert rows["frame"].tolist() == [0, 1] and rows["frame_clean"].tolist() == [1, 0] and rows["x0"].tolist() == [0, 31]
    assert rows["y0"].tolist() == [0, 15] and rows["ratio"].tolist() == [100.0, 250.0] and rows["flip"].tolist() == [0, 0]
    b.check(2, shape, **{**ok, "xy": [(32, 16), (3, 5)], "ratio": 300})
    for change in ({"xy": [(0, 0), (33, 16)]}, {"xy": [(0, 17), (0, 0)]}, {"xy": [(-1, 0), (0, 0)]}, {"xy": [(0, -1), (0, 0)]}, {"short": [0, 2]},
                   {"short": [-1, 0]}, {"long": [-1, 0]}, {"long": [0, 2]}, {"ratio": [0, 250]}, {"ratio": [-1, 250]}, {"ratio": [100, NAN]},
                   {"ratio": [100, math.inf]}, {"long": [0]}, {"xy": [(0, 0)]}):
        with pytest.raises(ValueError):
            b.check(2, shape, **{**ok, **change})
    for bad_shape in ((2, 63, 96), (2, 64, 95), (2, 30, 96), (64,)):
        with pytest.raises(ValueError):
            b.check(2, bad_shape, **ok)
    one = dd.DiffusionBatchBuilder(crop=1)
    one.check(1, (1, 4, 4), [0], [0], [(1, 1)], 100)
    for bad_shape in ((1, 2, 8), (1, 8, 2)):                  # a packed side of 1: the coordinates would divide by zero
        with pytest.raises(ValueError, match="sides of 2"):
            one.check(1, bad_shape, [0], [0], [(0, 0)], 100)
    g = dd.GenerationBatchBuilder(crop=16)
    rows = g.check(2, shape, [1, 0], [(0, 0), (32, 16)])[32:].view(raw.ROW)
    assert rows["frame"].tolist() == rows["frame_clean"].tolist() == [1, 0] and rows["ratio"].tolist() == [1.0, 1.0]
    for change in (dict(frame=[0, 2]), dict(frame=[-1, 0]), dict(xy=[(0, 0), (33, 16)]), dict(xy=[(0, 17), (0, 0)]), dict(frame=[0])):
        with pytest.raises(ValueError):
            g.check(2, shape, **{**dict(frame=[1, 0], xy=[(0, 0), (32, 16)]), **change})
    dk = dd.GenerationBatchBuilder(crop=16, dark_frame=True)
    rows = dk.check(2, (32, 48), None, [(0, 0), (32, 16)])[32:].view(raw.ROW)
    assert rows["x0"].tolist() == [0, 32] and rows["y0"].tolist() == [0, 16]
    for bad in (dict(shape=(32, 48), xy=[(0, 0), (33, 16)]), dict(shape=(2, 64, 96), xy=[(0, 0), (32, 16)]), dict(shape=(15, 48), xy=[(0, 0), (0, 0)])):
        with pytest.raises(ValueError):
            dk.check(2, bad["shape"], None, bad["xy"])
    cpu = torch.zeros(shape, dtype=torch.int16)
    with pytest.raises(L.HipError):
        b(cpu, **ok)
    with pytest.raises(L.HipError):
        g(cpu, [1, 0], [(0, 0), (32, 16)], [3, 4])
    with pytest.raises(L.HipError):
        dk((32, 48), None, [(0, 0)], 3, device="cpu")
    with pytest.raises(L.HipError):
        b.capture_inputs(2, "cpu")


def test_entry_point_refuses_each_bad_argument_without_a_gpu():
    from noisediff_amd import _lib as L
    lib = L.load()
    f, odd, odd4 = C.c_void_p(4096), C.c_void_p(4098), C.c_void_p(4100)      # never dereferenced: every call below fails its checks first

    def call(frames=f, N=2, H2=64, W2=96, table=f, black=512.0, white=16383.0, noise=f, noisy=f, clean=f, coord=f, B=2, h=16, w=24):
        return lib.nd_raw_diffusion_batch_f32(frames, N, H2, W2, table, black, white, noise, noisy, clean, coord, B, h, w, None)

    none = dict(noise=None, noisy=None, clean=None, coord=None)
    assert call(H2=63) == -1 and call(W2=95) == -1 and call(H2=0) == -1
    assert call(H2=2, h=1) == -1 and b"sides of 2" in lib.nd_last_error()
    assert call(W2=2, w=1) == -1
    assert call(h=0) == -1 and call(w=0) == -1 and call(B=0) == -1 and call(h=-1) == -1 and call(B=65536) == -1
    assert call(h=33) == -1 and call(w=49) == -1
    assert call(table=None) == -1 and b"table" in lib.nd_last_error()
    assert call(**none) == -1 and b"at least one" in lib.nd_last_error()
    for name in ("noise", "noisy", "clean"):
        assert call(frames=None, **{**none, name: f}) == -1 and b"need the frames" in lib.nd_last_error()
        assert call(N=0, **{**none, name: f}) == -1
    assert call(frames=odd) == -1 and call(table=odd4) == -1
    for name in none:
        assert call(**{name: odd}) == -1 and b"aligned" in lib.nd_last_error()
    assert call(white=512.0) == -1 and call(black=-1.0) == -1 and call(white=70000.0) == -1


def test_balanced_sample_list_repeats_small_groups_in_first_seen_order():
    from noisediff_amd import diffusion_data as dd
    sizes = {(800, 100): 1, (1600, 250): 33, (25600, 300): 99, (3200, 100): 100, (800, 250): 150, (200, 300): 50}
    pairs, left = [], dict(sizes)
    i = 0
    while any(left.values()):                                 # the groups interleaved, as the train list has them
        for key in sizes:
            if left[key]:
                left[key] -= 1
                pairs.append((f"s{i}", f"l{i}", key[0], key[1] + (0.4 if key == (1600, 250) else 0.0)))      # int(ratio) is the key
                i += 1
    got = dd.balanced_sample_list(pairs)
    count = {}
    for e in got:
        count[(e[2], int(e[3]))] = count.get((e[2], int(e[3])), 0) + 1
    assert count == {(800, 100): 100, (1600, 250): 99, (25600, 300): 99, (3200, 100): 100, (800, 250): 150, (200, 300): 100}
    assert list(count) == list(sizes)                         # first-seen group order
    # the counting rule of dataset.py:72-80, transcribed
    table = {}
    for e in pairs:
        table.setdefault(str(int(e[2])) + "_" + str(int(e[3])), []).append(e)
    for key, value in table.items():
        if len(value) < 100 and len(value) > 0:
            table[key] = int(100. / len(value)) * value
    want = []
    for value in table.values():
        want.extend(value)
    assert got == want
    assert dd.balanced_sample_list([]) == []


def test_frame_batches_walk_the_patch_grid_in_order():
    from noisediff_amd import diffusion_data as dd, io
    g = dd.GenerationBatchBuilder(512)
    assert g.grid() == io.patch_grid(512) and len(g.grid()) == 24
    batches = list(g.frame_batches(3, 5))
    assert [len(xy) for _, xy in batches] == [5, 5, 5, 5, 4] and all(fr == [3] * len(xy) for fr, xy in batches)
    assert [p for _, xy in batches for p in xy] == io.patch_grid(512)
    assert g.grid()[0] == (0, 0) and g.grid()[-1] == (io.PACKED_W - 512, io.PACKED_H - 512) and g.grid()[1][1] == 0       # row-major: x runs first
    small = dd.GenerationBatchBuilder(32)
    assert small.grid((68, 104)) == io.patch_grid(32, 104, 68) and small.grid((68, 104)) != small.grid((104, 68))
    assert [p for _, xy in small.frame_batches(0, 4, (68, 104)) for p in xy] == io.patch_grid(32, 104, 68)
    with pytest.raises(ValueError):
        small.grid((31, 104))
    with pytest.raises(ValueError):
        next(small.frame_batches(0, 0))


# --------------------------------------------------------------------------- GPU

def _np(t):
    return t.detach().cpu().numpy()


def _dev_frames(frames):
    return torch.from_numpy(np.ascontiguousarray(frames).view(np.int16)).to(DEV)


def _rows(specs):
    """specs: (frame, frame_clean, x0, y0, ratio) per sample; the fields the kernel must not read are set to values that would show."""
    from noisediff_amd import raw
    rows = np.zeros(len(specs), raw.ROW)
    for r, (fr, fc, x0, y0, ratio) in zip(rows, specs):
        r["frame"], r["frame_clean"], r["x0"], r["y0"], r["ratio"] = fr, fc, x0, y0, ratio
        r["flip"], r["branch"], r["iso"], r["blc"], r["k"], r["sd"], r["ratio64"] = 1, 1, 25600.0, 3.0, NAN, NAN, NAN
    return rows


def _launch(fd, shape, rows, h, w, want=KEYS, pad=3, offset=0):
    """nd_raw_diffusion_batch_f32 into NaN-filled buffers `pad` samples longer than the kernel writes, the outputs starting `offset` floats into
    them; the outputs not in `want` are NULL.  Returns {name: numpy (B, C, h, w)} after checking that everything around the outputs is still NaN.
    fd: the frames on the device, or None (NULL)."""
    from noisediff_amd import _lib as L
    from noisediff_amd._host import _stream
    B = len(rows)
    N, H2, W2 = shape
    table = torch.from_numpy(rows.view(np.uint8)).to(DEV)
    bufs = {k: torch.full(((B + pad) * (2 if k == "coord" else 4) * h * w,), NAN, device=DEV) for k in want}
    ptrs = [bufs[k].data_ptr() + 4 * offset if k in bufs else None for k in KEYS]
    L.call("nd_raw_diffusion_batch_f32", L.ptr(fd), N, H2, W2, table.data_ptr(), 512.0, 16383.0, *ptrs, B, h, w, _stream(DEV))
    torch.cuda.synchronize()
    res = {}
    for k, t in bufs.items():
        a, n = _np(t), B * (2 if k == "coord" else 4) * h * w
        assert np.isnan(a[:offset]).all() and np.isnan(a[offset + n:]).all(), f"the kernel wrote outside {k}"
        res[k] = a[offset:offset + n].reshape(B, -1, h, w)
    return res


def _want(frames, spec, h, w):
    fr, fc, x0, y0, ratio = spec
    return D.sample(frames[fr], frames[fc], x0, y0, h, w, ratio)


def _check(got, b, frames, spec, h, w, what):
    want = _want(frames, spec, h, w)
    for k, a in got.items():
        assert a.dtype == np.float32 and np.array_equal(a[b], want[k]), f"{what} {k}: {int((a[b] != want[k]).sum())} of {want[k].size} elements differ"


@pytest.mark.gpu
def test_every_uint16_code():
    perm = np.argsort(synth.uniform01(5, "raw.t.codes", 65536), kind="stable").astype(np.uint16)
    assert np.array_equal(np.sort(perm), np.arange(65536, dtype=np.uint16))
    frames = np.stack([perm.reshape(256, 256), perm[::-1].reshape(256, 256)])
    fd = _dev_frames(frames)
    specs = [(0, 1, 0, 0, 1), (1, 0, 0, 0, 100), (0, 1, 0, 0, 250), (1, 0, 0, 0, 300)]
    got = _launch(fd, frames.shape, _rows(specs), 128, 128)
    for b, spec in enumerate(specs):
        _check(got, b, frames, spec, 128, 128, f"ratio {spec[4]}")
    assert float(got["clean_img"].max()) > 4 and float(got["noise"].min()) < -3 and set(np.unique(got["noisy_img"][1])) >= {0.0, 1.0}
    assert not np.isnan(got["noise"]).any()


ADDRESSING = {
    "whole_frame_vector_path": ((136, 208), 68, 104, [(0, 1, 0, 0, 100)]),
    "rows_off_16_bytes_and_odd_width": ((66, 94), 33, 47, [(1, 0, 0, 0, 300)]),
    "window_8_4": ((136, 208), 24, 40, [(0, 1, 8, 4, 250)]),
    "window_6_5": ((136, 208), 24, 40, [(1, 0, 6, 5, 100)]),
    "window_3_2": ((136, 208), 24, 40, [(0, 0, 3, 2, 300)]),
    "width_2_mod_4": ((136, 208), 24, 42, [(0, 1, 5, 7, 100)]),
    "two_workgroups_on_each_axis": ((136, 208), 36, 64, [(0, 1, 40, 32, 100), (1, 0, 7, 0, 300)]),       # 36 * 16 = 576 threads > 256
    "three_samples_of_two_frames": ((136, 208), 24, 40, [(0, 1, 8, 4, 100), (1, 0, 31, 17, 300), (1, 1, 64, 44, 250)]),
}


def _addr_frames(H2, W2):
    return np.floor(synth.uniform(9, f"raw.t.addr.{H2}", (2, H2, W2), 300.0, 2000.0).numpy()).astype(np.uint16)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(ADDRESSING))
def test_addressing_and_output_subsets(case):
    (H2, W2), h, w, specs = ADDRESSING[case]
    frames = _addr_frames(H2, W2)
    fd = _dev_frames(frames)
    full = None
    for want in SUBSETS:
        frameless = want == ("coord",)
        got = _launch(None if frameless else fd, frames.shape, _rows(specs), h, w, want)
        assert set(got) == set(want)
        for b, spec in enumerate(specs):
            _check(got, b, frames, spec, h, w, f"{case} {want} b {b}")
            alone = _launch(None if frameless else fd, frames.shape, _rows([spec]), h, w, want)
            assert all(np.array_equal(alone[k][0], got[k][b]) for k in want)                  # the batch does not matter
        full = got if full is None else full
        assert all(np.array_equal(got[k], full[k]) for k in want)                             # nor does what else was asked for


@pytest.mark.gpu
def test_outputs_off_16_bytes_take_the_narrower_forms():
    (H2, W2), h, w, specs = ADDRESSING["whole_frame_vector_path"]                             # w = 104 would allow four columns per thread
    frames = _addr_frames(H2, W2)
    fd = _dev_frames(frames)
    for offset in (1, 2):                                     # 4-byte aligned: one column per thread; 8-byte: two
        got = _launch(fd, frames.shape, _rows(specs), h, w, KEYS, offset=offset)
        _check(got, 0, frames, specs[0], h, w, f"offset {offset}")


@pytest.mark.gpu
def test_a_bad_table_row_gives_nan_for_that_sample_only():
    frames = _addr_frames(136, 208)
    fd = _dev_frames(frames)
    h, w, good = 24, 40, (0, 1, 8, 4, 100)
    windows = [(0, 1, 65, 4, 100), (0, 1, 8, 45, 100), (0, 1, -1, 4, 100), (0, 1, 8, -1, 100)]
    short, long = [(2, 1, 8, 4, 100), (-1, 1, 8, 4, 100)], [(0, 2, 8, 4, 100), (0, -1, 8, 4, 100)]
    for bad in windows + short + long:
        got = _launch(fd, frames.shape, _rows([good, bad, good]), h, w)
        assert all(np.isnan(got[k][1]).all() for k in KEYS), bad
        for b in (0, 2):
            _check(got, b, frames, good, h, w, f"next to {bad}")
    for bad in windows:                                       # a window outside the frame has no coordinates either
        got = _launch(None, frames.shape, _rows([good, bad]), h, w, ("coord",))
        assert np.isnan(got["coord"][1]).all()
        _check(got, 0, frames, good, h, w, f"coord next to {bad}")
    for bad in short:                                         # `frame` is read for noise and noisy_img only
        got = _launch(fd, frames.shape, _rows([good, bad]), h, w, ("clean_img", "coord"))
        _check(got, 1, frames, good, h, w, f"clean and coord with {bad}")
        got = _launch(fd, frames.shape, _rows([good, bad]), h, w, ("noisy_img", "coord"))
        assert np.isnan(got["noisy_img"][1]).all() and np.isnan(got["coord"][1]).all()
        _check(got, 0, frames, good, h, w, f"noisy next to {bad}")
    for bad in long:                                          # `frame_clean` for noise and clean_img only
        got = _launch(fd, frames.shape, _rows([good, bad]), h, w, ("noisy_img", "coord"))
        _check(got, 1, frames, good, h, w, f"noisy and coord with {bad}")
        got = _launch(fd, frames.shape, _rows([good, bad]), h, w, ("clean_img",))
        assert np.isnan(got["clean_img"][1]).all()
    got = _launch(None, frames.shape, _rows([short[0], long[1], (7, -3, 8, 4, 100)]), h, w, ("coord",))       # neither, with the coordinates alone
    for b in range(3):
        _check(got, b, frames, good, h, w, "coord with bad frame indices")


@pytest.mark.gpu
def test_coordinates_at_the_sid_geometry_need_no_frames(gold):
    H, W, c = 1424, 2128, 64
    specs = [(0, 0, 0, 0, 1), (0, 0, W - c, H - c, 1), (0, 0, 1000, H - c - 1, 1)]           # the corners, and the bottom band's y
    got = _launch(None, (0, 2 * H, 2 * W), _rows(specs), c, c, ("coord",))["coord"]
    for b, (_, _, x0, y0, _) in enumerate(specs):
        rows = np.arange(y0, y0 + c).astype(np.float32) / np.float32(H - 1)
        cols = np.arange(x0, x0 + c).astype(np.float32) / np.float32(W - 1)
        assert np.array_equal(got[b, 0], np.broadcast_to(rows[:, None], (c, c))) and np.array_equal(got[b, 1], np.broadcast_to(cols[None, :], (c, c)))
        assert np.array_equal(got[b, 0, :, 0], gold.z["sid.coord_rows"][y0:y0 + c]) and np.array_equal(got[b, 1, 0], gold.z["sid.coord_cols"][x0:x0 + c])
    assert got[1, 0, -1, 0] == 1 and got[1, 1, 0, -1] == 1 and got[0, 0, 0, 0] == 0 and got[2, 0, -1, 0] < 1


@pytest.mark.gpu
def test_public_builders_equal_the_reference_goldens(gold):
    from noisediff_amd import DiffusionBatchBuilder, GenerationBatchBuilder
    z, c = gold.z, gold.crop
    stack = np.stack([gold.frames["short"], gold.frames["long"]])
    xy = [tuple(int(v) for v in z[f"train.{i}.xy"]) for i in range(gold.n)]
    ratio = [gold.pairs[i % 3][1] for i in range(gold.n)]
    idx = [gold.mapping[i % 3] for i in range(gold.n)]
    tb = DiffusionBatchBuilder(c)
    batch = tb(stack, [0] * gold.n, [1] * gold.n, xy, ratio, idx, want=KEYS)
    assert set(batch) == set(KEYS) | {"iso_ratio_idx"} and batch["iso_ratio_idx"].dtype == torch.int64 and batch["iso_ratio_idx"].device == DEV
    assert batch["iso_ratio_idx"].tolist() == idx
    for i in range(gold.n):
        for key in KEYS:
            assert np.array_equal(_np(batch[key])[i], z[f"train.{i}.{key}"]), (i, key)
    default = tb(_dev_frames(stack), [0] * gold.n, [1] * gold.n, xy, ratio)                   # a device tensor; the default outputs; no index
    assert set(default) == {"noise", "clean_img", "coord"} and all(torch.equal(default[k], batch[k]) for k in default)
    cond = tb.condition(batch)
    assert set(cond) == {"clean_img", "iso_ratio_idx", "position"} and cond["position"] is batch["coord"] and cond["clean_img"] is batch["clean_img"]
    gb, dk = GenerationBatchBuilder(c), GenerationBatchBuilder(c, dark_frame=True)
    gen = gb(stack, [1] * len(gold.patches), gold.patches, 31)
    dark = dk((gold.H, gold.W), None, gold.patches, [31] * len(gold.patches))
    assert set(gen) == set(dark) == {"clean_img", "position", "iso_ratio_idx", "image_coord"}
    assert gen["image_coord"] == dark["image_coord"] == [f"{x}_{y}" for x, y in gold.patches]
    assert gen["iso_ratio_idx"].tolist() == dark["iso_ratio_idx"].tolist() == [31] * len(gold.patches) and gen["iso_ratio_idx"].dtype == torch.int64
    for j in range(len(gold.patches)):
        assert np.array_equal(_np(gen["clean_img"])[j], z[f"gen.{j}.clean_img"]) and np.array_equal(_np(gen["position"])[j], z[f"gen.{j}.coord"])
    assert torch.equal(dark["position"], gen["position"]) and dark["clean_img"].shape == gen["clean_img"].shape and not dark["clean_img"].any()
    walked = [p for _, pts in gb.frame_batches(1, 4, (gold.H, gold.W)) for p in pts]         # the frame's own grid, batch by batch
    pos = torch.cat([gb(stack, fr, pts, 31)["position"] for fr, pts in gb.frame_batches(1, 4, (gold.H, gold.W))])
    assert len(walked) == pos.shape[0] == len(gb.grid((gold.H, gold.W)))
    for (x, y), p in zip(walked, _np(pos)):
        assert np.array_equal(p, D.coord(gold.H, gold.W, x, y, c, c))


@pytest.mark.gpu
def test_captured_launches_replay_with_rewritten_tables():
    """One launch in each graph; the device block is rewritten between replays."""
    from noisediff_amd import diffusion_data as dd
    frames = np.floor(synth.uniform(9, "raw.t.graph", (2, 136, 208), 300.0, 4000.0).numpy()).astype(np.uint16)
    fd = _dev_frames(frames)
    shape, c = tuple(fd.shape), 32
    tb, gb, dk = dd.DiffusionBatchBuilder(c), dd.GenerationBatchBuilder(c), dd.GenerationBatchBuilder(c, dark_frame=True)
    t1 = dict(short=[0, 1], long=[1, 0], xy=[(0, 0), (72, 36)], ratio=[100, 300])
    t2 = dict(short=[1, 1], long=[0, 0], xy=[(7, 3), (21, 35)], ratio=[250, 100])
    g1, g2 = dict(frame=[0, 1], xy=[(0, 0), (72, 36)]), dict(frame=[1, 1], xy=[(5, 9), (41, 2)])
    ti, gi, di = tb.capture_inputs(2, DEV), gb.capture_inputs(2, DEV), dk.capture_inputs(2, DEV)
    tb.update(ti, shape, **t1)
    gb.update(gi, shape, **g1)
    dk.update(di, (68, 104), None, g1["xy"])
    tout = {k: torch.empty(2, 2 if k == "coord" else 4, c, c, device=DEV) for k in KEYS}
    gout = {k: torch.empty(2, n, c, c, device=DEV) for k, n in (("clean_img", 4), ("position", 2))}
    dout = {"position": torch.empty(2, 2, c, c, device=DEV)}

    launches = [(lambda: tb.launch(ti, fd, tout, want=KEYS), tout), (lambda: gb.launch(gi, fd, gout), gout), (lambda: dk.launch(di, (68, 104), dout), dout)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for fn, _ in launches:
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graphs = []
    for fn, bufs in launches:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            res = fn()
        graphs.append(g)
        assert set(res) == set(bufs) and all(res[k] is bufs[k] for k in bufs)                # the launch wrote into what it was given
    for tp, gp in ((t1, g1), (t2, g2), (t1, g2)):
        tb.update(ti, shape, **tp)
        gb.update(gi, shape, **gp)
        dk.update(di, (68, 104), None, gp["xy"])
        for t in list(tout.values()) + list(gout.values()) + list(dout.values()):
            t.fill_(NAN)
        for g in graphs:
            g.replay()
        torch.cuda.synchronize()
        want_t, want_g = tb(fd, **tp, want=KEYS), gb(fd, gp["frame"], gp["xy"], 0)
        assert all(torch.equal(tout[k], want_t[k]) for k in KEYS)
        assert all(torch.equal(gout[k], want_g[k]) for k in gout) and torch.equal(dout["position"], want_g["position"])
        for b in range(2):
            ref = D.sample(frames[tp["short"][b]], frames[tp["long"][b]], *tp["xy"][b], c, c, tp["ratio"][b])
            assert all(np.array_equal(_np(tout[k])[b], ref[k]) for k in KEYS)


@pytest.mark.gpu
def test_a_training_step_and_a_generation_run_on_batches_from_raw_frames(gold):
    from noisediff_amd import GaussianDiffusion, NoiseDiffNet, TrainableNoiseDiffNet, diffusion_data as dd, io, train
    from util import state_dict
    dim, c, B = 16, 32, 2                                     # the smallest width and crop of the GPU training tests (test_trainable.py)
    fd = _dev_frames(np.stack([gold.frames["short"], gold.frames["long"]]))
    tb = dd.DiffusionBatchBuilder(c)
    state = np.random.get_state()
    try:
        np.random.seed(3)
        prm = tb.random_params(B, (gold.H, gold.W))
    finally:
        np.random.set_state(state)
    batch = tb(fd, [0] * B, [1] * B, prm["xy"], [100, 300], [7, 74])
    assert batch["noise"].shape == (B, 4, c, c) and torch.isfinite(batch["noise"]).all() and float(batch["noise"].std()) > 0
    net = TrainableNoiseDiffNet(SimpleNamespace(dim=dim))
    net.load_state_dict(state_dict(dim), strict=True)
    net = net.to(DEV).hip()
    gd = GaussianDiffusion(net, image_size=c, timesteps=1000, beta_schedule="sigmoid2", objective="pred_v").to(DEV)
    opt = train.Adam(net.parameters(), lr=1e-4)
    opt.zero_grad(set_to_none=True)
    loss = gd(batch["noise"], condition=tb.condition(batch))
    loss.backward()
    grads = [p.grad for p in net.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads)
    opt.step()
    torch.cuda.synchronize()
    assert math.isfinite(float(loss.detach())) and float(loss.detach()) > 0

    gb = dd.GenerationBatchBuilder(c)
    frame, xy = next(gb.frame_batches(1, B, (gold.H, gold.W)))
    cond = gb(fd, frame, xy, 31)
    sampler = NoiseDiffNet(SimpleNamespace(dim=dim, cond_dim=4, inp_dim=4, self_condition=False, normalize_condition=False))
    sampler.load_state_dict(state_dict(dim), strict=True)
    sampler = sampler.to(DEV).eval()
    gs = GaussianDiffusion(sampler, image_size=c, timesteps=1000, sampling_timesteps=3, beta_schedule="sigmoid2").to(DEV)
    out = gs.sample(batch_size=B, condition=cond, seed=11)
    noisy = io.compose_noisy(out, cond["clean_img"])
    assert out.shape == noisy.shape == cond["clean_img"].shape == (B, 4, c, c) and torch.isfinite(out).all() and torch.isfinite(noisy).all()
    assert cond["image_coord"] == [io.image_coord(x, y) for x, y in xy]
