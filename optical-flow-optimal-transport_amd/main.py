"""Drop-in for the reference's ``main.py`` CLI (main.py:27-148): same flags, same stdout,
same output files (.flo, benchmark txt, reconstruction / luminosity PNGs).  The solvers run
on the GPU; ``--device`` and ``--cg-mode`` are additions.

    python main.py frame10.png frame11.png --algo=foto --Nt=16 --r=1 \
        --convergence-tol=0.01 --reg-epsilon=1e-2 --max-it=200 --out=foto.flo
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
from PIL import Image  # noqa: E402

import utils  # noqa: E402
import benamou_brenier  # noqa: E402
import classical  # noqa: E402


def build_parser():
    p = argparse.ArgumentParser(description="sample argument parser")
    p.add_argument("f0", help="first frame")
    p.add_argument("f1", help="second frame")
    p.add_argument("--out", nargs="?", help="optical flow output")
    p.add_argument("--ground-truth", nargs="?", help="optical flow ground truth")
    p.add_argument("--save-benchmark", nargs="?", help="file output of benchmark")
    p.add_argument("--save-reconstruction", nargs="?", help="file output of reconstruction")
    p.add_argument("--save-lum", nargs="?", help="file output of luminosity")
    p.add_argument("--algo", nargs="?", help="Algorithm")
    p.add_argument("--Nt", nargs="?", type=int, default=4, help="Discretization in time")
    p.add_argument("--r", nargs="?", type=float, default=1., help="augmented langrangian parameter")
    p.add_argument("--convergence-tol", nargs="?", type=float, default=0.1, help="Stopping threshold")
    p.add_argument("--reg-epsilon", nargs="?", type=float, default=1e-3,
                   help="Regularization for the step 1 of Benamou-Brenier")
    p.add_argument("--max-it", nargs="?", type=int, default=100, help="Maximal number of iteration")
    p.add_argument("--normalize", action=argparse.BooleanOptionalAction, help="normalize the input images if enabled")
    p.add_argument("--alpha", nargs="?", type=float, default=0.1, help="Horn-Schunck alpha")
    p.add_argument("--lambdaa", nargs="?", type=float, default=0.2, help="Horn-Schunck lambda")
    # additions
    p.add_argument("--device", type=int, default=-1, help="HIP device ordinal (default: current)")
    p.add_argument("--cg-mode", type=int, default=None, help="0 stencil, 1 spectral, 2 spectral s-step, 3 Gauss-compressed spectral CG (default)")
    p.add_argument("--gn-levels", type=int, default=1, help="GN: pyramid levels (1: the reference's single solve)")
    p.add_argument("--gn-warps", type=int, default=1, help="GN: warped increment solves per pyramid level")
    p.add_argument("--tv-lambda", type=float, default=38.0, help="TVL1: data weight, for frames in [0, 1]")
    p.add_argument("--tv-theta", type=float, default=0.3, help="TVL1: coupling of the flow and its auxiliary")
    p.add_argument("--tv-tau", type=float, default=0.25, help="TVL1: dual step")
    p.add_argument("--tv-gamma", type=float, default=0.1, help="TVL1: illumination coupling (0: the channel is off)")
    p.add_argument("--tv-levels", type=int, default=4, help="TVL1: pyramid levels")
    p.add_argument("--tv-warps", type=int, default=5, help="TVL1: linearisations per pyramid level")
    p.add_argument("--tv-iters", type=int, default=30, help="TVL1: inner iterations per warp")
    p.add_argument("--sk-eps", type=float, default=2.0,
                   help="sinkhorn: the entropic regularisation, the variance of the Gaussian kernel in px^2")
    p.add_argument("--sk-radius", type=int, default=16, help="sinkhorn: the kernel's window radius in px (0..32)")
    p.add_argument("--sk-iters", type=int, default=100, help="sinkhorn: iterations (a fixed count, no stop test)")
    p.add_argument("--inbetweens", type=int, default=0,
                   help="FOTO: motion-compensated in-betweens of the two input frames at this many evenly spaced "
                        "interior times (0: none)")
    p.add_argument("--save-inbetweens", default=None,
                   help="FOTO: prefix of the in-between PNGs, written as PREFIX001.png, PREFIX002.png, ...")
    p.add_argument("--stats", action="store_true",
                   help="with --ground-truth: also the robustness R0.5 / R1.0 / R2.0 and the accuracy percentiles "
                        "A50 / A75 / A95 of EE, and the AE twins (R2.5 / R5.0 / R10.0, degrees), after the "
                        "reference's lines")
    p.add_argument("--save-consistency", default=None,
                   help="file output of the forward-backward consistency mask (255 = consistent); the backward flow "
                        "is the solved transport read backwards (FOTO) or a second solve with the frames swapped "
                        "(GN); also prints the four class counts")
    p.add_argument("--median", type=int, default=0, choices=range(0, 8), metavar="R",
                   help="radius R (1..7) of a weighted median of the solved flow, guided by frame 0, applied before "
                        "the flow is written and evaluated (0: none)")
    p.add_argument("--median-rounds", type=int, default=1, choices=range(1, 65), metavar="N",
                   help="rounds of --median (1..64)")
    p.add_argument("--fill-occluded", action="store_true",
                   help="mask the flow by the forward-backward check of --save-consistency (the --median, if any, then "
                        "ignores the rejected pixels) and fill the rejected pixels from their neighbours; prints the "
                        "filled and unfilled counts")
    p.add_argument("--resize", default=None, metavar="S|WxH",
                   help="prepare the frames on the device before the solve: resized by the factor S, or to W x H, "
                        "with PIL's Image.resize arithmetic (run.sh:18-30 halves them: --resize 0.5)")
    p.add_argument("--resize-filter", default="lanczos", choices=("box", "bilinear", "bicubic", "lanczos"),
                   help="filter of --resize")
    p.add_argument("--normalize-pair", action="store_true",
                   help="prepare the frames on the device before the solve: the mass equalisation of "
                        "bin/normalize_image.py (run.sh:50-70), quantised to 8 bits like its PNGs")
    p.add_argument("--flow-full-size", action="store_true",
                   help="with --resize: resize the solved flow back to the size of the input frames (bilinear, u and "
                        "v scaled with it) before --out, --stats and the --save-* outputs")
    p.add_argument("--lk", type=int, default=0, metavar="K",
                   help="also track the K strongest Shi-Tomasi corners of frame 0 with pyramidal Lucas-Kanade (0: "
                        "none); with --ground-truth prints the mean EE of the tracks and of the solved flow at the "
                        "same corners")
    p.add_argument("--lk-radius", type=int, default=7, choices=range(1, 8), metavar="R", help="LK: window radius (1..7)")
    p.add_argument("--lk-levels", type=int, default=4, help="LK: pyramid levels")
    p.add_argument("--lk-iters", type=int, default=10, help="LK: iterations per level")
    p.add_argument("--lk-check", action="store_true",
                   help="LK: the forward-backward check (status bit 8: the round trip misses the corner by more than "
                        "half a pixel)")
    p.add_argument("--match", type=int, default=0, metavar="K",
                   help="instead of --lk: match the K strongest corners of frame 0 to those of frame 1 by binary "
                        "descriptors (foto.match: no limit on the displacement; 0: none); with --global-motion also "
                        "fits the model to the matches")
    p.add_argument("--match-orientations", type=int, default=1, metavar="N",
                   help="match: orientation bins of the descriptor (1: upright; 32 follows a roll of the camera)")
    p.add_argument("--match-ratio", type=float, default=0.8, help="match: Lowe's ratio (0: no ratio test)")
    p.add_argument("--match-max-disp", type=float, default=0.0, metavar="PX",
                   help="match: only corners within PX pixels in x and in y are candidates (0: no gate)")
    p.add_argument("--match-patch", type=int, default=15, metavar="R", help="match: the descriptor's radius (2..31)")
    p.add_argument("--save-tracks", default=None, metavar="FILE",
                   help="with --lk or --match: one text row per corner, `x y dx dy status err` (--match: err is the "
                        "best Hamming distance)")
    p.add_argument("--global-motion", default=None, choices=("translation", "similarity", "affine", "homography"),
                   metavar="MODEL", help="fit the solved flow with one parametric motion (translation, similarity, "
                   "affine, homography; foto.motion.fit_flow on every fourth pixel, --save-consistency's mask when "
                   "that is computed) and print its matrix and inlier share")
    p.add_argument("--save-residual-flow", default=None, metavar="FILE",
                   help="with --global-motion: the flow minus the model's field, as .flo")
    return p


def global_motion(w, h, u, v, model, mask=None):
    """The solved flow fitted by ``model`` on the device: (matrix (3, 3), inliers, usable lattice
    pixels, residual u, residual v).  ``mask``: uint8 (h * w), non-zero = usable."""
    from foto import device as D
    from foto import motion
    flow = D.DeviceArray.from_numpy(np.stack([np.reshape(u, (h, w)), np.reshape(v, (h, w)),
                                              np.zeros((h, w))]).astype(np.float64))
    dm = None if mask is None else D.DeviceArray.from_numpy(np.reshape(mask, (h, w)).astype(np.uint8))
    fit = motion.fit_flow(flow, w, h, mask=dm, model=model)
    res = motion.residual(flow, fit).to_numpy()
    inliers, usable, _, _ = fit.counts()
    return fit.matrix(), inliers, usable, res[0].reshape(-1), res[1].reshape(-1)


def lk_tracks(f0, f1, w, h, K, radius=7, levels=4, iters=10, check=False):
    """(points, disp, status, err) of --lk K as numpy arrays: foto.device.lk_track on the two frames
    (float64 in [0, 1], as utils.openGrayscaleImage returns them)."""
    from foto import device as D
    a, b = (D.DeviceArray.from_numpy(np.asarray(f, dtype=np.float64).reshape(h, w)) for f in (f0, f1))
    res = D.lk_track(a, b, int(K), check=check, dtype="float64", radius=radius, levels=levels, iters=iters)
    return tuple(x.to_numpy() for x in res[:4])


def match_tracks(f0, f1, w, h, K, model=None, orientations=1, ratio=0.8, max_disp=0.0, patch=15):
    """(points, disp, status, best distance) of --match K as numpy arrays, the rows of frame 0's
    corners: foto.device.match_frames on the two frames, mutual check included; with ``model`` the
    matches are fitted too (foto.motion.fit): (matrix (3, 3), inliers, usable matches) after them."""
    from foto import device as D
    from foto import motion
    a, b = (D.DeviceArray.from_numpy(np.asarray(f, dtype=np.float64).reshape(h, w)) for f in (f0, f1))
    pts, disp, status, _, dist = D.match_frames(a, b, int(K), dtype="float64", orientations=orientations,
                                                ratio=ratio if ratio > 0 else None, max_disp=max_disp, patch=patch)
    fit = motion.fit(pts, disp, w, h, model, status=status) if model else None
    p = pts.to_numpy()
    rows = np.isfinite(p).all(axis=1)   # (the rows beyond the corner count are NaN)
    res = (p[rows], disp.to_numpy()[rows], status.to_numpy()[rows], dist.to_numpy()[rows, 0].astype(np.float64))
    if fit is not None:
        inliers, usable, _, _ = fit.counts()
        res += (fit.matrix(), inliers, usable)
    return res


def flows_at(points, w, h, *flows):
    """Each (u, v) of ``flows`` read at the corners: foto.sparse.sample on one buffer, (R, M, 2)."""
    from foto import device as D
    from foto import sparse
    z = np.zeros((h, w))
    buf = np.stack([np.stack([np.asarray(u, dtype=np.float64).reshape(h, w),
                              np.asarray(v, dtype=np.float64).reshape(h, w), z]) for u, v in flows])
    pts = D.DeviceArray.from_numpy(np.ascontiguousarray(points, dtype=np.float64))
    return sparse.sample(D.DeviceArray.from_numpy(buf), pts).to_numpy()


UNKNOWN_FLOW_THRESH = 1e9   # Middlebury's marker (flowIO)


def track_rows(points, disp, status, err):
    """The rows of --save-tracks: `x y dx dy status err`, floats by repr."""
    return [" ".join([repr(float(p[0])), repr(float(p[1])), repr(float(d[0])), repr(float(d[1])), str(int(s)),
                      repr(float(e))]) for p, d, s, e in zip(points, disp, status, err)]


def _write_lines(lines, path):
    with open(path, "w") as f:
        f.write("".join(line + "\n" for line in lines))


def prepared_frames(args, size):
    """(f, w, h) x 2 of --resize / --normalize-pair: the input files as the decoder gives them (grey or
    RGB uint8), prepared on the device by foto.device.prepare_pair, back as utils.openGrayscaleImage
    returns a frame.  ``size`` None: not resized."""
    from foto import device as D
    up = [D.DeviceArray.from_numpy(_open_u8(p)) for p in (args.f0, args.f1)]
    out = []
    for d in D.prepare_pair(up[0], up[1], size=size, filter=args.resize_filter, normalize=args.normalize_pair):
        a = d.to_numpy()
        out.append((a.flatten() / 255, a.shape[1], a.shape[0]))
    return out


def resized_u8(a, size, filt):
    """A uint8 frame, grey or colour, through foto.prep.resize on the device."""
    from foto import device as D
    from foto import prep
    return prep.resize(D.DeviceArray.from_numpy(a), size, filt).to_numpy()


def flow_to_size(u, v, m, w, h, W, H):
    """The solved (u, v, m) of a w x h solve at W x H: foto.prep.resize_flow, bilinear."""
    from foto import device as D
    from foto import prep
    flow = np.stack([np.asarray(x, dtype=np.float64).reshape(h, w) for x in (u, v, m)])
    big = prep.resize_flow(D.DeviceArray.from_numpy(flow), (W, H), "bilinear").to_numpy()
    return big[0].reshape(-1), big[1].reshape(-1), big[2].reshape(-1)


def stats_lines(w, h, u, v, uGT, vGT):
    """The extra benchmark lines of --stats, as (name, value) pairs: foto.evaluate.score_flow on the
    solved flow and the .flo payload, AE in degrees."""
    from foto import evaluate
    flow = np.stack([np.asarray(x, dtype=np.float64).reshape(h, w) for x in (u, v, np.zeros(w * h))])
    gt = np.ascontiguousarray(np.stack([uGT, vGT], axis=-1).reshape(h, w, 2))
    s = evaluate.score_flow(flow, gt)
    deg = s.ae_degrees()
    lines = [(f"EE-R{t}", r) for t, r in zip(s.ee_thresholds, s.ee_R)]
    lines += [(f"EE-A{p:g}", a) for p, a in zip(s.percentiles, s.ee_A)]
    lines += [(f"AE-R{d}", r) for d, r in zip((2.5, 5.0, 10.0), s.ae_R)]
    lines += [(f"AE-A{p:g}", a) for p, a in zip(s.percentiles, deg["A"])]
    return [(k, float(x)) for k, x in lines]


def consistency_mask(w, h, u, v, bu, bv):
    """(255 * valid as uint8 (h, w), the four class counts) of the forward flow (u, v) against the
    backward flow (bu, bv): foto.chain.consistency with its default thresholds."""
    from foto import chain
    z = np.zeros((h, w))
    fwd = np.stack([np.asarray(x, dtype=np.float64).reshape(h, w) for x in (u, v)] + [z])
    bwd = np.stack([np.asarray(x, dtype=np.float64).reshape(h, w) for x in (bu, bv)] + [z])
    valid, table = chain.consistency(fwd, bwd)
    return np.uint8(255) * valid, [int(c) for c in table]


MEDIAN_SIGMA_R = 0.08     # the range term of --median / --fill-occluded, of the [0, 1] grey scale
FILL_RADIUS = 2           # --fill-occluded without --median


def median_tables(radius):
    """The weight tables of --median R: a Gaussian of sigma R in space, of MEDIAN_SIGMA_R in grey value."""
    from foto import filter as flt
    return flt.tables(radius, sigma_s=float(radius), sigma_r=MEDIAN_SIGMA_R)


def postprocess_flow(w, h, u, v, f0, radius=0, rounds=1, valid=None):
    """(u, v, counts) after --median / --fill-occluded: foto.filter.median of the solved flow guided
    by frame 0 (``radius`` > 0), masked by ``valid`` when given, then foto.filter.fill of what
    ``valid`` rejects; counts = (filled, unfilled) with a mask, else None."""
    from foto import filter as flt
    flow = np.stack([np.asarray(x, dtype=np.float64).reshape(h, w) for x in (u, v, np.zeros(w * h))])
    guide = np.asarray(f0, dtype=np.float64).reshape(h, w)
    usable = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
    if radius > 0:
        sp, rg = median_tables(radius)
        flow, usable, _ = flt.median(flow, guide=guide, mask=usable, radius=radius, rounds=rounds, spatial=sp, range=rg)
    counts = None
    if valid is not None:
        r = radius if radius > 0 else FILL_RADIUS
        sp, rg = median_tables(r)
        flow, usable, _ = flt.fill(flow, usable, guide=guide, radius=r, spatial=sp, range=rg)
        rejected = np.asarray(valid) == 0
        counts = (int(np.count_nonzero(rejected & (usable != 0))), int(np.count_nonzero(usable == 0)))
    return flow[0].reshape(-1), flow[1].reshape(-1), counts


def _save_gray(img, w, h, path):
    Image.fromarray(img.reshape([h, w]), "L").save(path)


def _open_u8(path):
    """An input frame as the caller has it: uint8 (h, w) for a grey-scale file, (h, w, 3) RGB otherwise."""
    im = Image.open(path)
    return np.asarray(im if im.mode == "L" else im.convert("RGB"), dtype=np.uint8)


def inbetween_times(K, Nt):
    """K evenly spaced interior plane positions of [0, Nt - 1]: neither input frame is among them."""
    return np.linspace(0.0, float(Nt - 1), int(K) + 2)[1:-1]


def main(argv=None, writer=None):
    """``writer``: an executor (run.py passes a one-thread pool) that takes the output-file
    writes (.flo, PNGs) off this thread, so the encoding overlaps the next solve; the files
    are the same.  None: written here, before main returns, as the reference does."""
    args = build_parser().parse_args(argv)

    def emit(fn, *a):
        if writer is None:
            fn(*a)
        else:
            writer.submit(fn, *a)

    np.random.seed(0)
    if args.flow_full_size and not args.resize:
        raise SystemExit("--flow-full-size needs --resize: there is no other size to come back from")
    if args.save_residual_flow and not args.global_motion:
        raise SystemExit("--save-residual-flow needs --global-motion: there is no model to remove")
    if args.lk > 0 and args.match > 0:
        raise SystemExit("--lk and --match are two ways to the same tracks: choose one")
    full = None
    if args.resize or args.normalize_pair:   # (off by default: every other run reads its frames as before)
        (f1, w, h), (f2, w, h) = prepared_frames(args, args.resize)
        if args.flow_full_size:
            full = prepared_frames(args, None)
    else:
        f1, w, h = utils.openGrayscaleImage(args.f0)
        f2, w, h = utils.openGrayscaleImage(args.f1)
    sw, sh = w, h   # (the size of the solve: w, h become the full size under --flow-full-size)

    print("***********************************")
    print("Input images: ")
    print(" - f0 = " + str(args.f0) + " / total mass = " + str(np.sum(f1)))
    print(" - f1 = " + str(args.f1) + " / total mass = " + str(np.sum(f2)))
    if args.normalize is True:
        print(" - normalize input images")
        rho1 = f1 / (np.sum(f1))
        rho2 = f2 / (np.sum(f2))
    else:
        rho1 = f1
        rho2 = f2

    start_time = time.time()
    if args.algo == "foto":
        print(" - algorithm: FOTO")
        print(f"\t - Nt={args.Nt}")
        print(f"\t - r={args.r}")
        print(f"\t - convergence_tol={args.convergence_tol}")
        print(f"\t - reg_epsilon={args.reg_epsilon}")
        print(f"\t - max_it={args.max_it}")
        opts = {"device": args.device}
        if args.cg_mode is not None:
            opts["cg_mode"] = args.cg_mode
        inbetweens, backward = [], []
        if args.inbetweens > 0 and args.save_inbetweens:   # (on the solved context, after the flow extraction)
            c0, c1 = _open_u8(args.f0), _open_u8(args.f1)
            if args.resize:   # (the in-betweens are drawn at the size of the solve)
                c0, c1 = (resized_u8(c, args.resize, args.resize_filter) for c in (c0, c1))
            opts["then"] = lambda s: inbetweens.append(s.interpolate(c0, c1, inbetween_times(args.inbetweens, args.Nt)))
        if args.save_consistency or args.fill_occluded:   # (the a-planes of the maps at the last plane: frame 1 -> frame 0, a - p)
            first = opts.get("then")

            def then(s):
                if first is not None:
                    first(s)
                backward.append(s.maps([args.Nt - 1])[0, :2])

            opts["then"] = then
        u, v, m = benamou_brenier.solve(rho1, rho2, args.Nt, w, h, r=args.r, convergence_tol=args.convergence_tol,
                                        reg_epsilon=args.reg_epsilon, max_it=args.max_it, **opts)
    elif args.algo == "GN":
        print(" - algorithm: GN")
        print(f"\t - alpha={args.alpha}")
        print(f"\t - lambda={args.lambdaa}")
        gn = classical.GLLOpticalFlow(w, h)
        gn.setAlpha(args.alpha)
        gn.setLambda(args.lambdaa)
        if (args.gn_levels, args.gn_warps) != (1, 1):
            print(f"\t - pyramid: {args.gn_levels} levels x {args.gn_warps} warps")
            gn.setPyramid(args.gn_levels, args.gn_warps)
        [u, v, m] = gn.assemble(rho1, rho2).process()
    elif args.algo == "TVL1":
        from foto import tvl1
        tv = dict(lam=args.tv_lambda, theta=args.tv_theta, tau=args.tv_tau, gamma=args.tv_gamma, levels=args.tv_levels,
                  warps=args.tv_warps, iters=args.tv_iters)
        print(" - algorithm: TVL1")
        for name in ("lambda", "theta", "tau", "gamma", "levels", "warps", "iters"):
            print(f"\t - {name}={tv['lam' if name == 'lambda' else name]}")
        solver = tvl1.cached_tvl1(w, h, **tv)
        u, v, m, _ = solver.solve(rho1, rho2)
    elif args.algo == "sinkhorn":
        from foto import sinkhorn
        print(" - algorithm: sinkhorn")
        print(f"\t - eps={args.sk_eps}")
        print(f"\t - radius={args.sk_radius}")
        print(f"\t - iters={args.sk_iters}")
        solver = sinkhorn.cached_sinkhorn(w, h, args.sk_eps, args.sk_radius)
        u, v, m = solver.solve(rho1, rho2, args.sk_iters)
    else:
        # reference: `assert("not implemented")` (always true), then NameError on `u` below
        raise NotImplementedError(f"algorithm {args.algo!r} is not implemented (use --algo=foto, --algo=GN, "
                                  "--algo=TVL1 or --algo=sinkhorn)")
    timer = time.time() - start_time

    checked = []

    def cross_check(fu, fv):
        """(mask, counts) of the solved flow against its backward flow, computed once."""
        if not checked:
            if args.algo == "GN":   # (after the timer: the second solve is not part of the benchmark)
                bu, bv, _ = gn.assemble(rho2, rho1).process()
            elif args.algo == "TVL1":
                bu, bv, _, _ = solver.solve(rho2, rho1)
            elif args.algo == "sinkhorn":
                bu, bv, _ = solver.solve(rho2, rho1, args.sk_iters)
            else:
                bu, bv = backward[0]
            checked.append(consistency_mask(sw, sh, fu, fv, bu, bv))
        return checked[0]

    solved = (u, v)
    if args.median > 0 or args.fill_occluded:   # (the flow written and evaluated below is the filtered one)
        valid = (cross_check(*solved)[0] != 0) if args.fill_occluded else None
        u, v, counts = postprocess_flow(w, h, u, v, f1, args.median, args.median_rounds, valid)
        if args.median > 0:
            print(f" - median filter: radius {args.median}, {args.median_rounds} round(s), guided by f0")
        if counts is not None:
            print(" - occluded pixels filled / unfilled: " + " / ".join(str(c) for c in counts))

    if full is not None:   # (the consistency mask stays at the size of the solve, sw x sh)
        (F1, W, H), (F2, _, _) = full
        print(f" - flow resized from {w}x{h} to {W}x{H}")
        u, v, m = flow_to_size(u, v, m, w, h, W, H)
        f1, f2, w, h = F1, F2, W, H

    print("Benchmark:")
    rec = utils.apply_opticalflow(f1, u, v, w, h, m)
    rec = np.clip(rec, 0, 1)
    IE = utils.IE(w, h, rec, f2)
    print(" - time: " + str(timer) + "s")
    print(" - IE: " + str(IE))

    if args.ground_truth:
        wGT, hGT, uGT, vGT = utils.openFlo(args.ground_truth)
        assert wGT == w and hGT == h
        AEE, SDEE = utils.EE(w, h, u, v, uGT, vGT)
        AAE, SDAE = utils.AE(w, h, u, v, uGT, vGT)
        print(" - EE-mean: " + str(AEE))
        print(" - EE-stddev: " + str(SDEE))
        print(" - AE-mean: " + str(AAE))
        print(" - AE-stddev: " + str(SDAE))
        extra = stats_lines(w, h, u, v, uGT, vGT) if args.stats else []
        for name, x in extra:
            print(" - " + name + ": " + str(x))

    if args.lk > 0:
        pts, disp, status, err = lk_tracks(f1, f2, w, h, args.lk, args.lk_radius, args.lk_levels, args.lk_iters,
                                           args.lk_check)
        print(f" - LK: {len(pts)} corners tracked (radius {args.lk_radius}, {args.lk_levels} levels, "
              f"{args.lk_iters} iterations)")
        if args.lk_check:
            print(" - LK forward-backward inconsistent: " + str(int(np.count_nonzero(status & 8))))
        if args.ground_truth:
            gt, dense = flows_at(pts, w, h, (uGT, vGT), (u, v))
            known = ~((np.abs(gt) > UNKNOWN_FLOW_THRESH).any(axis=1) | np.isnan(gt).any(axis=1))
            print(" - LK corners with known truth: " + str(int(known.sum())))
            if known.any():
                print(" - LK EE-mean at the corners: " + str(float(np.hypot(*(disp - gt)[known].T).mean())))
                print(f" - {args.algo} EE-mean at the corners: " + str(float(np.hypot(*(dense - gt)[known].T).mean())))
        if args.save_tracks:
            print("saving tracks...")
            emit(_write_lines, track_rows(pts, disp, status, err), args.save_tracks)

    if args.match > 0:
        res = match_tracks(f1, f2, w, h, args.match, args.global_motion, args.match_orientations, args.match_ratio,
                           args.match_max_disp, args.match_patch)
        pts, disp, status, err = res[:4]
        print(f" - match: {int(np.count_nonzero(status == 0))} of {len(pts)} corners matched (patch "
              f"{args.match_patch}, {args.match_orientations} orientations, ratio {args.match_ratio})")
        if args.global_motion:
            print(f" - match motion ({args.global_motion}): " + " ".join(repr(float(x)) for x in res[4].ravel()) +
                  " / inlier share: " + str(res[5] / max(res[6], 1)))
        if args.save_tracks:
            print("saving tracks...")
            emit(_write_lines, track_rows(pts, disp, status, err), args.save_tracks)

    if args.global_motion:
        # (the mask is of the solved flow at the size of the solve: it serves a flow of that size)
        gm_mask = cross_check(*solved)[0] if args.save_consistency and (sw, sh) == (w, h) else None
        gm, gm_in, gm_usable, ru, rv = global_motion(w, h, u, v, args.global_motion, gm_mask)
        print(f" - global motion ({args.global_motion}): " + " ".join(repr(float(x)) for x in gm.ravel()) +
              " / inlier share: " + str(gm_in / max(gm_usable, 1)))
        if args.save_residual_flow:
            print("saving residual flo file...")
            emit(utils.saveFlo, w, h, ru, rv, args.save_residual_flow)

    if args.save_benchmark:
        with open(args.save_benchmark, "w") as f:
            if args.ground_truth:
                f.write("EE-mean: " + str(AEE) + "\n")
                f.write("EE-stddev: " + str(SDEE) + "\n")
                f.write("AE-mean: " + str(AAE) + "\n")
                f.write("AE-stddev: " + str(SDAE) + "\n")
            f.write("IE: " + str(IE) + "\n")
            f.write("time: " + str(timer) + "s")
            if args.ground_truth and args.stats:   # (after the reference's lines, whose last has no newline)
                for name, x in extra:
                    f.write("\n" + name + ": " + str(x))

    if args.out:
        print("saving flo file...")
        emit(utils.saveFlo, w, h, u, v, args.out)

    if args.save_reconstruction:
        print("saving reconstruction...")
        emit(_save_gray, np.uint8(255 * rec), w, h, args.save_reconstruction)

    if args.save_lum:
        print("saving luminosity...")
        emit(_save_gray, np.uint8(255 * np.clip((m + 1) / 2, 0, 1)), w, h, args.save_lum)

    if args.save_consistency:
        print("saving consistency mask...")
        mask, counts = cross_check(*solved)   # (of the solved flow, before any --median)
        print(" - consistent / inconsistent / leaves the frame / not finite: " + " / ".join(str(c) for c in counts))
        emit(_save_gray, mask, sw, sh, args.save_consistency)

    if args.algo == "foto" and inbetweens:
        print("saving in-betweens...")
        for k, img in enumerate(inbetweens[0]):
            emit(lambda a, path: Image.fromarray(a).save(path), img, f"{args.save_inbetweens}{k + 1:03d}.png")

    print("***********************************")
    return u, v, m


if __name__ == "__main__":
    main()
