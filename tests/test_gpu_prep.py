"""Frame preparation on the device (include/foto.h, "frame preparation") against tests/prep_ref.py,
the numpy restatement that tests/test_prep_host.py pins to Pillow's Image.resize / convert('L') and
to the bin/ tools.

Bar.  Every stage is defined operation by operation (integer arithmetic for uint8, a float64
accumulator in tap order for the floats, IEEE divisions for the pointwise stages), so every
comparison is on BIT PATTERNS: no tolerance is involved.  The one inexact quantity is the frame sum
of the pair normalisation, a fixed-order reduction in another order than math.fsum: |S - fsum(f)| <=
n 2^-53 fsum(f) bounds any summation order of n non-negative terms (tests/test_gpu_device.py's
bound); the normalised frames are then recomputed in numpy FROM the returned sums, bit for bit.

Sizes.  The horizontal pass works on tiles of TX = prep.TILE_X = 64 outputs and stages up to 512
input elements per tile row on chip; output widths 1, TX - 1, TX, TX + 1, 2 TX + 3 sit on the tile
seams, 640 -> 7 has one tile that spans all 640 inputs (the direct-read route), 131 -> 65 runs both
routes.  Everything else is the smallest frame with an odd size and more than one block."""
import math

import numpy as np
import pytest

from conftest import PKG, REPO  # noqa: F401

import prep_ref as R
from foto import device as D
from foto import prep

pytestmark = pytest.mark.gpu

U8, F32, F64 = np.uint8, np.float32, np.float64
DTYPES = (U8, F32, F64)
TX = prep.TILE_X
HOST_SHAPES = [((53, 37), (26, 18)), ((53, 37), (27, 19)), ((64, 40), (32, 20)), ((29, 31), (58, 62)),
               ((29, 31), (17, 45)), ((16, 16), (7, 16)), ((200, 9), (3, 9)), ((7, 5), (1, 1))]


def dev(a):
    return D.DeviceArray.from_numpy(a)


def frame(shape, dtype, seed):
    """uint8 noise, or floats beyond [0, 1] with both signs (Lanczos then over- and undershoots)."""
    rng = np.random.default_rng(seed)
    if dtype == U8:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    return (rng.random(shape) * 300 - 20).astype(dtype)


def padded(a, pad=5):
    """(device view, host array): the frame as the left part of wider rows (stride_y = w + pad)."""
    wide = np.zeros(a.shape[:1] + (a.shape[1] + pad,) + a.shape[2:], a.dtype)
    wide[:, :a.shape[1]] = a
    return dev(wide)[:, :a.shape[1]]


def sources(h, w, dtype, seed):
    """The two kinds of source every resize case runs on, as (host array, device view): a row-padded
    grey frame (stride_y > w) and an interleaved RGB one (stride_x = 3, stride_c = 1)."""
    g, rgb = frame((h, w), dtype, seed), frame((h, w, 3), dtype, seed + 1000)
    return [(g, padded(g)), (rgb, dev(rgb))]


def check_resize(a, size, filt, d=None, **kw):
    got = prep.resize(dev(a) if d is None else d, size, filt, **kw).to_numpy()
    R.same_bits(got, R.resize(a, size, filt))
    return got


# ------------------------------------------------------------------ resize

@pytest.mark.parametrize("src,dst", HOST_SHAPES)
def test_resize_matches_pil_restatement(src, dst):
    """All four filters and all three dtypes: a row-padded grey source and an interleaved RGB one."""
    (w, h), size = src, dst
    for k, dtype in enumerate(DTYPES):
        for a, d in sources(h, w, dtype, 10 + k):
            for filt in prep.FILTERS:
                check_resize(a, size, filt, d)


@pytest.mark.parametrize("ow", [1, TX - 1, TX, TX + 1, 2 * TX + 3])
def test_resize_tile_seams(ow):
    """Output widths on the seams of the horizontal tiles, from a 2x larger source and from a 0.5x
    smaller one; five rows: more than one row group, the last one partial."""
    for w in (2 * ow, max(1, ow // 2)):
        for k, dtype in enumerate(DTYPES):
            for a, d in sources(5, w, dtype, 30 + k):
                for filt in prep.FILTERS:
                    check_resize(a, (ow, 5), filt, d)


def test_resize_direct_route_at_a_large_reduction():
    """640 -> 7: 551 Lanczos taps per output, one tile spanning all 640 inputs with every filter:
    beyond the staging, so the automatic route reads directly and the forced LDS route is refused."""
    plan = prep.cached_plan(640, 5, 7, 5, "lanczos")
    info = plan.info()
    assert info["ksize_x"] == 551 and info["span_x"] == 640
    for k, dtype in enumerate(DTYPES):
        for a, d in sources(5, 640, dtype, 40 + k):
            for filt in prep.FILTERS:
                check_resize(a, (7, 5), filt, d)
                check_resize(a, (7, 5), filt, d, route="direct")
    with pytest.raises(prep._lib.FotoError, match="ROUTE_LDS"):
        plan.resize(dev(frame((5, 640), U8, 1)), route="lds")


def test_resize_both_routes_equal_bits():
    for k, dtype in enumerate(DTYPES):
        for a, d in sources(18, 131, dtype, 50 + k):
            for filt in prep.FILTERS:
                lds = check_resize(a, (65, 9), filt, d, route="lds")
                direct = check_resize(a, (65, 9), filt, d, route="direct")
                R.same_bits(lds, direct)


@pytest.mark.parametrize("size", [(23, 30), (40, 17)])
def test_resize_one_pass_alone(size):
    """Only w changes (the horizontal pass writes the output), only h changes (the vertical pass
    reads the strided source)."""
    for k, dtype in enumerate(DTYPES):
        a = frame((30, 40), dtype, 60 + k)
        check_resize(a, size, "bicubic", padded(a))
        rgb = frame((30, 40, 3), dtype, 63 + k)
        check_resize(rgb, size, "lanczos")


def test_resize_equal_sizes_returns_the_input_bits():
    for k, dtype in enumerate(DTYPES):
        a = frame((29, 37), dtype, 70 + k)
        if dtype != U8:
            a[3, 4], a[5, 6] = np.nan, -0.0
        R.same_bits(prep.resize(padded(a), (37, 29), "lanczos").to_numpy(), a)


def test_resize_planar_channels():
    """A (C, h, w) frame gives (C, oh, ow), all channels in one call; also from a view whose planes
    are every second one of a larger array (stride_c = 2 h w)."""
    for k, dtype in enumerate(DTYPES):
        a = frame((6, 21, 34), dtype, 75 + k)
        got = prep.resize(dev(a)[::2], (17, 11), "bicubic", channels_last=False).to_numpy()
        R.same_bits(got, np.stack([R.resize2d(a[c], (17, 11), "bicubic") for c in (0, 2, 4)]))
        got = prep.resize(dev(a), (34, 9), "lanczos", channels_last=False).to_numpy()   # the vertical pass alone
        R.same_bits(got, np.stack([R.resize2d(a[c], (34, 9), "lanczos") for c in range(6)]))


# ------------------------------------------------------------------ grey

def test_gray():
    h, w = 33, 41
    rgb, rgba = frame((h, w, 3), U8, 80), frame((h, w, 4), U8, 81)
    R.same_bits(prep.gray(dev(rgb)).to_numpy(), R.gray(rgb))
    R.same_bits(prep.gray(dev(rgba)).to_numpy(), R.gray(rgba))
    planar = frame((3, h, w), F64, 82)
    R.same_bits(prep.gray(dev(planar), channels_last=False).to_numpy(), R.gray(np.moveaxis(planar, 0, 2)))
    f32 = frame((h, w, 3), F32, 83)
    R.same_bits(prep.gray(dev(f32)).to_numpy(), R.gray(f32))


# ------------------------------------------------------------------ flow resize

def flow(R_, h, w, layout, dtype, seed):
    rng = np.random.default_rng(seed)
    shape = (R_, 3, h, w) if layout == "planar" else (R_, h, w, 2)
    return (rng.standard_normal(shape) * 3).astype(dtype)


@pytest.mark.parametrize("dtype,layout", [(F32, "interleaved"), (F64, "planar")])
def test_flow_resize(dtype, layout):
    f = flow(3, 14, 20, layout, dtype, 90)
    for filt in ("bilinear", "bicubic"):
        got = prep.resize_flow(dev(f), (41, 29), filt, layout=layout).to_numpy()
        R.same_bits(got, R.resize_flow(f, layout, (41, 29), filt))
    one = prep.resize_flow(dev(f[0]), (41, 29), "bilinear", layout=layout).to_numpy()   # no record axis
    R.same_bits(one, R.resize_flow(f[:1], layout, (41, 29), "bilinear")[0])


def test_flow_resize_constant_flow_doubles_exactly():
    f = np.empty((1, 3, 14, 20), F64)
    f[0, 0], f[0, 1], f[0, 2] = 2.0, -1.0, 0.25
    got = prep.resize_flow(dev(f), 2.0, "bilinear").to_numpy()
    assert got.shape == (1, 3, 28, 40)
    assert np.all(got[0, 0] == 4.0) and np.all(got[0, 1] == -2.0) and np.all(got[0, 2] == 0.25)
    fi = np.empty((14, 20, 2), F32)
    fi[..., 0], fi[..., 1] = 2.0, -1.0
    goti = prep.resize_flow(dev(fi), (40, 28), "bilinear", layout="interleaved").to_numpy()
    assert np.all(goti[..., 0] == 4.0) and np.all(goti[..., 1] == -2.0)


# ------------------------------------------------------------------ pair normalisation

@pytest.mark.parametrize("dtype", [U8, F64])
@pytest.mark.parametrize("w,h", [(96, 80), (7, 3)])
def test_normalize_pair(dtype, w, h):
    rng = np.random.default_rng(100 + w)
    if dtype == U8:
        f0, f1 = frame((h, w), U8, 101), frame((h, w), U8, 102)
    else:
        f0, f1 = rng.random((h, w)), rng.random((h, w)) * 0.5
    for out_dtype in ("uint8", "float64", "float32"):
        o0, o1, st = prep.normalize_pair(padded(f0), dev(f1), dtype=out_dtype)
        n = w * h
        for S, f in ((st["S0"], f0), (st["S1"], f1)):
            exact = math.fsum(R.values(f).ravel())
            print(f"sum: device {S!r}, fsum {exact!r}, |diff| {abs(S - exact):.3e}, bound {n * 2.0 ** -53 * exact:.3e}")
            assert abs(S - exact) <= n * 2.0 ** -53 * exact
        w0, w1, (m0, m1) = R.normalize_pair(f0, f1, st["S0"], st["S1"], out_dtype)
        assert (st["max0"], st["max1"]) == (m0, m1)
        R.same_bits(o0.to_numpy(), w0)
        R.same_bits(o1.to_numpy(), w1)


# ------------------------------------------------------------------ illumination and difference

BORDER_SHAPES = [("rect", 20, 10, 5, 3, 0.125),      # over the left and top borders
                 ("rect", 30, 30, 60, 40, -0.2),     # over the right and bottom borders
                 ("rect", 7, 5, 30, 20, 0.3),        # odd extents: int(r - L / 2) truncates
                 ("circle", 9.5, 0, 0, 0.25),        # centred on a corner
                 ("circle", 12.0, 63, 47, -0.15),
                 ("circle", 200.0, 32, 24, 0.01),    # covers the frame
                 ("rect", 200, 200, 32, 24, -0.02),
                 ("circle", 0.5, 10, 10, 0.5)]       # one pixel


def test_illuminate():
    w, h = 64, 48
    for src in (frame((h, w), U8, 110), np.random.default_rng(111).random((h, w))):
        for shapes in (prep.lum_shapes(w, h, 12345), BORDER_SHAPES, []):
            for out_dtype in ("uint8", "float64"):
                got = prep.illuminate(padded(src), shapes, dtype=out_dtype).to_numpy()
                R.same_bits(got, R.illuminate(src, shapes, out_dtype))


def test_difference():
    w, h = 64, 48
    a8, b8 = frame((h, w), U8, 120), frame((h, w), U8, 121)
    a, b = np.random.default_rng(122).random((h, w)), np.random.default_rng(123).random((h, w))
    for f0, f1 in ((a8, b8), (a, b)):
        for out_dtype in ("uint8", "float32", "float64"):
            got, (mn, mx) = prep.difference(dev(f0), padded(f1), dtype=out_dtype, return_minmax=True)
            R.same_bits(got.to_numpy(), R.difference(f0, f1, out_dtype))
            d = R.values(f1) - R.values(f0)
            assert (mn, mx) == (d.min(), d.max())


def test_difference_constant_is_zero_over_zero():
    f0 = frame((48, 64), U8, 130)
    assert not prep.difference(dev(f0), dev(f0.copy()), dtype="uint8").to_numpy().any()
    assert np.isnan(prep.difference(dev(f0), dev(f0.copy()), dtype="float64").to_numpy()).all()
    g = np.random.default_rng(131).random((48, 64)).astype(F32)
    assert np.isnan(prep.difference(dev(g), dev(g.copy()), dtype="float32").to_numpy()).all()


# ------------------------------------------------------------------ prepare_pair

def _textured_rgb(h, w, shift, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 120 + 80 * np.sin((xx - shift) / 5.0) * np.cos(yy / 7.0)
    return np.clip(base[..., None] + rng.integers(-10, 11, (h, w, 3)), 0, 255).astype(U8)


def test_prepare_pair_then_bb_flow():
    """prepare_pair (grey, Lanczos halving, pair normalisation) followed by bb_flow equals bb_flow
    on the frames prepared by the restatement, bit for bit."""
    c0, c1 = _textured_rgb(48, 64, 0, 140), _textured_rgb(48, 64, 2, 141)
    p0, p1 = D.prepare_pair(dev(c0), dev(c1), size=0.5)
    r0, r1 = (R.resize(R.gray(c), (32, 24), "lanczos") for c in (c0, c1))
    _, _, st = prep.normalize_pair(dev(r0), dev(r1))
    w0, w1, _ = R.normalize_pair(r0, r1, st["S0"], st["S1"], "uint8")
    R.same_bits(p0.to_numpy(), w0)
    R.same_bits(p1.to_numpy(), w1)
    kw = dict(Nt=4, max_it=3, convergence_tol=1e-9, dtype="float64")
    got = D.bb_flow(p0, p1, **kw).to_numpy()
    want = D.bb_flow(dev(w0), dev(w1), **kw).to_numpy()
    assert got.shape == (3, 24, 32)
    R.same_bits(got, want)
    # grey frames, no resize, no normalisation: the frames come back as they are
    q0, q1 = D.prepare_pair(dev(r0), dev(r1), normalize=False)
    R.same_bits(q0.to_numpy(), r0)


_TORCH_CHILD = r"""
import sys
sys.path[:0] = [{repo!r}, {pkg!r}, {tests!r}]
import torch                      # first: libfoto then binds to torch's HIP runtime
import numpy as np
import prep_ref as R
from foto import device, prep
rng = np.random.default_rng(7)
c0 = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
c1 = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
t0, t1 = torch.from_numpy(c0).cuda(), torch.from_numpy(c1).cuda()
p0, p1 = device.prepare_pair(t0, t1, size=(26, 18), normalize=False)
for p, c in ((p0, c0), (p1, c1)):
    got = torch.as_tensor(p, device="cuda").cpu().numpy()
    R.same_bits(got, R.resize(R.gray(c), (26, 18), "lanczos"))
f = torch.from_numpy((rng.standard_normal((3, 37, 53)) * 2).astype(np.float32)).cuda()
up = torch.as_tensor(prep.resize_flow(f, (106, 74), "bilinear"), device="cuda").cpu().numpy()
R.same_bits(up, R.resize_flow(f.cpu().numpy()[None], "planar", (106, 74), "bilinear")[0])
torch.cuda.synchronize()
print("TORCH CHILD OK")
"""


def test_torch_producer():
    import os
    import subprocess
    import sys
    code = _TORCH_CHILD.format(repo=REPO, pkg=PKG, tests=os.path.join(REPO, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240, env=dict(os.environ))
    assert r.returncode == 0 and "TORCH CHILD OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ------------------------------------------------------------------ main.py and run.py

def _colour_pngs(tmp_path, w, h):
    from PIL import Image
    paths = []
    for k, shift in enumerate((0, 2)):
        paths.append(str(tmp_path / f"c{k}.png"))
        Image.fromarray(_textured_rgb(h, w, shift, 150 + k), "RGB").save(paths[-1])
    return paths


def _quiet_main(argv):
    import contextlib
    import io
    import main as M
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = M.main(argv)
    return res, buf.getvalue()


def test_cli_resize_normalize_and_flow_full_size(tmp_path):
    """main.py --resize 0.5 --normalize-pair --flow-full-size on colour PNGs solves on the frames the
    restatement prepares and returns that flow resized back by the restatement, bit for bit."""
    from PIL import Image
    w, h = 64, 48
    paths = _colour_pngs(tmp_path, w, h)
    c = [np.asarray(Image.open(p).convert("RGB")) for p in paths]
    r0, r1 = (R.resize(R.gray(x), (32, 24), "lanczos") for x in c)
    _, _, st = prep.normalize_pair(dev(r0), dev(r1))
    prepared = []
    for k, a in enumerate(R.normalize_pair(r0, r1, st["S0"], st["S1"], "uint8")[:2]):
        prepared.append(str(tmp_path / f"p{k}.png"))
        Image.fromarray(a, "L").save(prepared[-1])
    (u, v, m), plain = _quiet_main(prepared + ["--algo=GN"])
    (U, V, M_), out = _quiet_main(paths + ["--algo=GN", "--resize", "0.5", "--normalize-pair", "--flow-full-size",
                                           f"--out={tmp_path / 'full.flo'}", f"--save-consistency={tmp_path / 'c.png'}"])
    _, checked = _quiet_main(prepared + ["--algo=GN", f"--save-consistency={tmp_path / 'c_small.png'}"])
    line = [l for l in checked.splitlines() if "not finite:" in l]
    assert line and line == [l for l in out.splitlines() if "not finite:" in l]     # the mask of the solve, at its size
    assert np.array_equal(np.asarray(Image.open(str(tmp_path / "c.png"))), np.asarray(Image.open(str(tmp_path / "c_small.png"))))
    assert Image.open(str(tmp_path / "c.png")).size == (32, 24)
    assert " - flow resized from 32x24 to 64x48" in out and "flow resized" not in plain
    small = np.stack([np.asarray(x, F64).reshape(24, 32) for x in (u, v, m)])[None]
    want = R.resize_flow(small, "planar", (w, h), "bilinear")[0]
    for got, ref in zip((U, V, M_), want):
        R.same_bits(np.asarray(got, F64).reshape(h, w), ref)
    import utils
    wf, hf, uf, vf = utils.openFlo(str(tmp_path / "full.flo"))
    assert (wf, hf) == (w, h) and np.array_equal(np.asarray(uf, F32).ravel(), want[0].astype(F32).ravel())


def test_run_prepare_device_writes_the_restatement_files(tmp_path):
    import types
    from PIL import Image
    import run
    w, h = 40, 30
    seq = tmp_path / "middlebury-1" / "eval-data-gray" / "Seq"
    seq.mkdir(parents=True)
    src = [frame((h, w), U8, 160 + k) for k in (0, 1)]
    for k, a in enumerate(src):
        Image.fromarray(a, "L").save(str(seq / f"frame1{k}.png"))
    args = types.SimpleNamespace(data=str(tmp_path), dataset=None, device=True)
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        run.prepare(args)
    half = [R.resize(a, (20, 15), "lanczos") for a in src]
    lum1 = R.illuminate(half[1], prep.lum_shapes(20, 15, run.bash_random(12345, 1)[0]), "uint8")
    for name, pair in (("middlebury-1", half), ("middlebury-1-lum", [half[0], lum1])):
        _, _, st = prep.normalize_pair(dev(pair[0]), dev(pair[1]))
        want = R.normalize_pair(pair[0], pair[1], st["S0"], st["S1"], "uint8")[:2]
        for k in (0, 1):
            got = np.asarray(Image.open(str(tmp_path / name / "eval-data-gray" / "Seq" / f"frame1{k}.png")))
            R.same_bits(got, want[k])


def test_cli_resize_with_inbetweens(tmp_path):
    """--resize with --inbetweens: the colour frames the in-betweens are drawn from are resized with
    the same filter, so they match the solver's size."""
    from PIL import Image
    paths = _colour_pngs(tmp_path, 64, 48)
    prefix = str(tmp_path / "ib")
    _, out = _quiet_main(paths + ["--algo=foto", "--Nt=4", "--max-it=3", "--resize", "32x24", "--resize-filter", "bicubic",
                                  "--inbetweens", "1", f"--save-inbetweens={prefix}"])
    assert "saving in-betweens..." in out
    im = Image.open(prefix + "001.png")
    assert im.size == (32, 24) and im.mode == "RGB"
