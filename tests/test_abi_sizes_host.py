"""The size rules of the C ABI, one table: every entry of include/foto.h that takes a grid or an
image size, at every degenerate size class -- an axis of 0, an axis of 1, w h = 2^31 -- and at the
smallest accepted size where the entry needs no device for it.  Argument checks precede any device
use, so this runs on a machine without a GPU.

The expected codes are literals, recorded from the build before the size checks were gathered into
image_size_check / grid_size_check (csrc/foto_host.cpp).  That build gives the same code for every
row (205 of 224) but the 19 marked `NEW` below, all of the w h = 2^31 class: entries whose plane
size had no w h < 2^31 rule (foto_grad_st, foto_div_st, foto_laplacian_st, foto_apply_A, foto_bb_rhs,
foto_cg, foto_flow_from_phi, foto_bb_create, foto_bb_create_dev, foto_bb_solve, foto_bb_solve_ex,
foto_gn_plan_create, foto_gn_solve_prior, foto_warp, foto_flow_errors, foto_intensity_error and the
three evaluation *_dev entries) went on to the device, whose kernels index pixels with 32 bits; on
a machine without a device they returned FOTO_ERR_HIP there.  Both shared checks apply the rule,
so these rows now return FOTO_ERR_ARG before any device use.

RUN: an accepted size that does need a device (the one-pixel-wide images of the entries whose
minimum side is 1).  It is past the argument checks: 0 with a device, FOTO_ERR_HIP without one."""
import ctypes

import numpy as np
import pytest

from foto import _lib

ARG, HIP, RUN = _lib.FOTO_ERR_ARG, -2, "run"
NEW = ARG   # (the rows the docstring lists)

_buf = np.zeros(4096)          # every pointer argument: large enough for every size that runs
_ints = (ctypes.c_int * 32)()
_i64 = (ctypes.c_int64 * 64)()


def _d():
    return _lib.dptr(_buf)


def _p():
    return ctypes.c_void_p(_buf.ctypes.data)


def _image(w):
    return _lib.Image(_buf.ctypes.data, _lib.FOTO_F64, max(w, 1), 1, 1.0)


def _flow():
    return _lib.Flow(_buf.ctypes.data, _lib.FOTO_F64, 0, 1)


def _handle():
    return ctypes.byref(ctypes.c_void_p())


# entry -> call(L, *sizes); grid entries take (Nt, Nx, Ny), image entries (w, h)
GRID = {
    "foto_grad_st": lambda L, t, x, y: L.foto_grad_st(_d(), t, x, y, _d()),
    "foto_div_st": lambda L, t, x, y: L.foto_div_st(_d(), t, x, y, _d()),
    "foto_laplacian_st": lambda L, t, x, y: L.foto_laplacian_st(_d(), t, x, y, _d()),
    "foto_apply_A": lambda L, t, x, y: L.foto_apply_A(_d(), t, x, y, 1.0, 1e-2, _d()),
    "foto_bb_rhs": lambda L, t, x, y: L.foto_bb_rhs(_d(), _d(), _d(), _d(), t, x, y, 1.0, _d()),
    "foto_cg": lambda L, t, x, y: L.foto_cg(_d(), t, x, y, 1.0, 1e-2, 1e-6, 10, 0, _d(), _ints),
    "foto_flow_from_phi": lambda L, t, x, y: L.foto_flow_from_phi(_d(), t, x, y, _d(), _d(), _d()),
    "foto_flow_path_from_phi": lambda L, t, x, y: L.foto_flow_path_from_phi(_d(), t, x, y, _d(), _d(), _d()),
    "foto_track_from_phi": lambda L, t, x, y: L.foto_track_from_phi(_d(), t, x, y, _d(), 2, 0, _d()),
    "foto_report_from_state": lambda L, t, x, y: L.foto_report_from_state(_d(), _d(), _d(), _d(), t, x, y, _d()),
    "foto_bb_create": lambda L, t, x, y: L.foto_bb_create(_d(), _d(), t, x, y, 1.0, 1e-2, None, _handle()),
    "foto_bb_solve": lambda L, t, x, y: L.foto_bb_solve(_d(), _d(), t, x, y, 1.0, 0.01, 1e-2, 2, _lib.ITER_CB(), None,
                                                        _d(), _d(), _d()),
    "foto_bb_solve_ex": lambda L, t, x, y: L.foto_bb_solve_ex(_d(), _d(), t, x, y, 1.0, 0.01, 1e-2, 2, None, _d(), _d(),
                                                              _d(), None, None),
    "foto_bb_create_dev": lambda L, t, x, y: L.foto_bb_create_dev(ctypes.byref(_image(x)), ctypes.byref(_image(x)), 0,
                                                                  None, t, x, y, 1.0, 1e-2, None, None, _handle()),
    # (kind FOTO_XFER_HALO = 0, one rank: host only)
    "foto_xfer_calls": lambda L, t, x, y: L.foto_xfer_calls(0, t, y, x, 1, 0, 0, _i64, 8, _ints),
}
IMAGE = {
    "foto_grad2": lambda L, w, h: L.foto_grad2(_d(), w, h, b"N", _d()),
    "foto_div2": lambda L, w, h: L.foto_div2(_d(), w, h, b"D", _d()),
    "foto_grad2_forward": lambda L, w, h: L.foto_grad2_forward(_d(), w, h, _d()),
    "foto_gn_apply": lambda L, w, h: L.foto_gn_apply(_d(), _d(), w, h, 0.1, 0.2, _d(), _d()),
    "foto_gn_rhs": lambda L, w, h: L.foto_gn_rhs(_d(), _d(), w, h, _d()),
    "foto_gn_solve": lambda L, w, h: L.foto_gn_solve(_d(), _d(), w, h, 0.1, 0.2, 1e-6, 10, _d(), _d(), _d(), _ints),
    "foto_gn_solve_ex": lambda L, w, h: L.foto_gn_solve_ex(_d(), _d(), w, h, 0.1, 0.2, 1e-6, 10, _d(), _d(), _d(), None),
    "foto_gn_plan_create": lambda L, w, h: L.foto_gn_plan_create(w, h, 0.1, 0.2, 1e-6, 10, _handle()),
    "foto_gn_pyr_sizes": lambda L, w, h: L.foto_gn_pyr_sizes(w, h, 3, 2, _ints, (ctypes.c_int * 16)(), 16,
                                                             ctypes.byref(ctypes.c_int())),
    "foto_gn_pyr_create": lambda L, w, h: L.foto_gn_pyr_create(w, h, 0.1, 0.2, None, _handle()),
    "foto_pyr_up(coarse)": lambda L, w, h: L.foto_pyr_up(_d(), _d(), _d(), w, h, 4, 4, _d(), _d(), _d()),
    "foto_pyr_up(fine)": lambda L, w, h: L.foto_pyr_up(_d(), _d(), _d(), 2, 2, w, h, _d(), _d(), _d()),
    "foto_gn_warp_prior": lambda L, w, h: L.foto_gn_warp_prior(_d(), _d(), _d(), _d(), w, h, _d()),
    "foto_gn_solve_prior": lambda L, w, h: L.foto_gn_solve_prior(_d(), _d(), w, h, 0.1, 0.2, 1e-6, 10, None, None, None,
                                                                 _d(), _d(), _d(), None),
    "foto_pyr_down": lambda L, w, h: L.foto_pyr_down(_d(), _d(), w, h, _d(), _d()),
    "foto_warp": lambda L, w, h: L.foto_warp(_d(), _d(), _d(), _d(), w, h, _d()),
    "foto_flow_errors": lambda L, w, h: L.foto_flow_errors(_d(), _d(), _d(), _d(), w, h, _d()),
    "foto_intensity_error": lambda L, w, h: L.foto_intensity_error(_d(), _d(), w, h, _d()),
    "foto_warp_dev": lambda L, w, h: L.foto_warp_dev(_p(), _p(), _p(), _p(), w, h, _p(), None),
    "foto_flow_errors_dev": lambda L, w, h: L.foto_flow_errors_dev(_p(), _p(), _p(), _p(), w, h, _d(), None),
    "foto_intensity_error_dev": lambda L, w, h: L.foto_intensity_error_dev(_p(), _p(), w, h, _d(), None),
    "foto_image_check": lambda L, w, h: L.foto_image_check(ctypes.byref(_image(w)), w, h),
    "foto_flow_check": lambda L, w, h: L.foto_flow_check(ctypes.byref(_flow()), w, h),
    "foto_render_warp_dev": lambda L, w, h: L.foto_render_warp_dev(ctypes.byref(_image(w)), 1, 1 << 40,
                                                                   ctypes.byref(_flow()), 0, w, h, _p(), _lib.FOTO_F64,
                                                                   None),
    "foto_render_lum_dev": lambda L, w, h: L.foto_render_lum_dev(ctypes.byref(_flow()), w, h, _p(), None),
    "foto_render_color_dev": lambda L, w, h: L.foto_render_color_dev(ctypes.byref(_flow()), w, h, 1.0, _p(), None, None),
}

G0 = [(0, 4, 4), (4, 0, 4), (4, 4, 0)]          # an axis of 0
G1 = [(1, 4, 4), (4, 1, 4), (4, 4, 1)]          # an axis of 1
GB = (2, 65536, 32768)                          # Nx Ny = 2^31
I0, I1, IB = [(0, 4), (4, 0)], [(1, 4), (4, 1)], (65536, 32768)

# (entry, sizes, expected)
CASES = []


def _rows(entry, sizes, codes):
    if not isinstance(sizes, list):
        sizes, codes = [sizes], [codes]
    elif not isinstance(codes, list):
        codes = [codes] * len(sizes)
    CASES.extend((entry, s, c) for s, c in zip(sizes, codes))


for _e in ("foto_grad_st", "foto_div_st", "foto_laplacian_st", "foto_apply_A", "foto_bb_rhs", "foto_cg",
           "foto_flow_from_phi", "foto_bb_create", "foto_bb_create_dev", "foto_bb_solve", "foto_bb_solve_ex"):
    _rows(_e, G0, ARG); _rows(_e, G1, ARG); _rows(_e, GB, NEW)
for _e in ("foto_flow_path_from_phi", "foto_track_from_phi"):
    _rows(_e, G0, ARG); _rows(_e, G1, ARG); _rows(_e, GB, ARG)
_rows("foto_report_from_state", G0, ARG); _rows("foto_report_from_state", G1, [ARG, RUN, RUN])
_rows("foto_report_from_state", GB, ARG)
# (the transfer lists: Nt, Ny >= world = 1 and Nx >= 1 -- no rule of the grid entries, host only)
_rows("foto_xfer_calls", G0, ARG); _rows("foto_xfer_calls", G1 + [(2, 2, 2)], 0)

for _e in ("foto_grad2", "foto_div2", "foto_grad2_forward", "foto_gn_apply", "foto_gn_rhs", "foto_gn_solve",
           "foto_gn_solve_ex", "foto_gn_pyr_create", "foto_pyr_up(coarse)", "foto_pyr_up(fine)", "foto_gn_warp_prior"):
    _rows(_e, I0, ARG); _rows(_e, I1, ARG); _rows(_e, IB, ARG)
for _e in ("foto_gn_plan_create", "foto_gn_solve_prior"):
    _rows(_e, I0, ARG); _rows(_e, I1, ARG); _rows(_e, IB, NEW)
_rows("foto_gn_pyr_sizes", I0, ARG); _rows("foto_gn_pyr_sizes", I1, ARG); _rows("foto_gn_pyr_sizes", IB, ARG)
_rows("foto_gn_pyr_sizes", (2, 2), 0)
_rows("foto_pyr_down", I0, ARG); _rows("foto_pyr_down", I1, RUN); _rows("foto_pyr_down", IB, ARG)
for _e in ("foto_warp", "foto_flow_errors", "foto_intensity_error"):
    _rows(_e, I0, ARG); _rows(_e, I1, RUN); _rows(_e, IB, NEW)
# (the *_dev entries need device pointers at an accepted size: only the rejected classes)
for _e in ("foto_warp_dev", "foto_flow_errors_dev", "foto_intensity_error_dev"):
    _rows(_e, I0, ARG); _rows(_e, IB, NEW)
# (host-only descriptor checks: their own rules, w, h >= 1 and no pixel-count limit)
for _e in ("foto_image_check", "foto_flow_check"):
    _rows(_e, I0, ARG); _rows(_e, I1 + [(1, 1), IB], 0)
for _e in ("foto_render_warp_dev", "foto_render_lum_dev", "foto_render_color_dev"):
    _rows(_e, I0, ARG)


def _id(case):
    return f"{case[0]}-{'x'.join(str(s) for s in case[1])}"


def test_table_covers_every_sized_entry():
    entries = {c[0].split("(")[0] for c in CASES}
    assert entries == {e.split("(")[0] for e in list(GRID) + list(IMAGE)}
    assert entries <= set(_lib.SIGNATURES)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_size_class(case):
    entry, sizes, expected = case
    L = _lib.lib()
    call = GRID.get(entry) or IMAGE[entry]
    rc = call(L, *sizes)
    msg = L.foto_last_error()
    print(entry, sizes, "->", rc, msg)
    if expected == RUN:
        n = ctypes.c_int(0)
        expected = 0 if L.foto_device_count(ctypes.byref(n)) == 0 and n.value > 0 else HIP
    assert rc == expected, msg
    if rc < 0:
        assert msg
