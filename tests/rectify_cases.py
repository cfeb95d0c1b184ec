"""The cameras of the lens rectification tests (tests/test_rectify_cpu.py, tests/test_gpu_rectify.py): plain numbers, each
a (Lens, width, height).  `simple(name)` is the same camera with R = I and P = [K | 0], for the round trips."""
import numpy as np

from dvs_mcemvs_amd import engine as E


def _K(fx, fy, cx, cy):
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def _rot_y(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])


def _rot_x(deg):
    a = np.deg2rad(deg)
    return np.array([[1.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a)], [0.0, np.sin(a), np.cos(a)]])


def _P(fx, fy, cx, cy, tx=0.0):
    return np.array([[fx, 0.0, cx, tx], [0.0, fy, cy, 0.0], [0.0, 0.0, 1.0, 0.0]])


_SPEC = {
    # 346 x 260 (DAVIS), a stereo-rectifying R and P: another focal length, and P[0][3] = -f * baseline, which is not read
    "plumb_bob_A": (E.LENS_PLUMB_BOB, 346, 260, _K(226.38, 226.15, 173.65, 133.73), (-0.09, 0.19, 8e-5, 2e-3),
                    _rot_y(2.0), _P(199.65, 199.65, 177.43, 126.81, -19.94)),
    # odd width, no multiple of 64, partial last workgroup, not square
    "plumb_bob_B": (E.LENS_PLUMB_BOB, 67, 45, _K(30.0, 30.0, 33.2, 21.7), (-0.6, 0.1, 0.0, 0.0, 0.0), None, None),
    # as B, with k2 = 0.05: 1 + k1 r2 + k2 r2^2 is negative for r2 in (2, 10), which B's (discriminant < 0) never is
    "plumb_bob_B2": (E.LENS_PLUMB_BOB, 67, 45, _K(30.0, 30.0, 33.2, 21.7), (-0.6, 0.05, 0.0, 0.0, 0.0), None, None),
    # 8 coefficients: the rational model's denominator is not 1
    "plumb_bob_C": (E.LENS_PLUMB_BOB, 97, 131, _K(110.0, 111.5, 47.3, 66.1), (-0.12, 0.03, 1e-3, -5e-4, -0.004, 0.02, 0.005, 0.001),
                    _rot_x(-1.5), _P(100.0, 100.0, 48.0, 65.0)),
    "fisheye_A": (E.LENS_FISHEYE, 1280, 720, _K(1050.3, 1049.1, 640.4, 359.7), (-0.04, 0.003, -0.002, 0.0003),
                  _rot_y(-1.2) @ _rot_x(0.4), _P(880.0, 880.0, 652.0, 371.0, -105.6)),
    # f = 12: theta_d passes pi / 2 at the corners; c on an integer pixel: theta_d = 0 there; the polynomial has a maximum,
    # so Newton finds no root for the outer pixels, and some iterates change sign
    "fisheye_B": (E.LENS_FISHEYE, 67, 45, _K(12.0, 12.0, 33.0, 22.0), (-0.3, 0.05, -0.01, 0.001), None, None),
}

NAMES = tuple(_SPEC)
PLUMB_BOB = tuple(n for n in NAMES if n.startswith("plumb_bob"))
FISHEYE = tuple(n for n in NAMES if n.startswith("fisheye"))


def camera(name):
    model, w, h, K, D, R, P = _SPEC[name]
    return E.Lens(model, K, D, R, P), w, h


def simple(name):
    model, w, h, K, D, _, _ = _SPEC[name]
    return E.Lens(model, K, D), w, h


def ulp32(v):
    """Spacing of float32 at |v|."""
    return float(np.spacing(np.float32(abs(v))))
