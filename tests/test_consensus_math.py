"""The per-lane arithmetic of the consensus estimators (sr_livo_amd/csrc/srl_consensus_math.h) compiled as plain C++ and run on the CPU:
tests/consensus_math_main.cpp, a stand-alone program with its own main, is built twice with the host compiler -- plain, and with
-fsanitize=address,undefined -- and every test below runs on both.  The sampler must be the contract's (tests/consensus_checker.py
restates it from the header's text), the root finders are held against np.roots on polynomials with chosen roots, the 7-point chain and
P3P against a known matrix and a known pose.  No device call, and nothing of Python in the instrumented process."""
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import consensus_checker as ck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("consensus_math") / request.param)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-o", out, os.path.join(ROOT, "tests", "consensus_math_main.cpp")]
    if request.param == "sanitized":
        cmd[5:5] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and ("cannot find -lasan" in b.stderr or "cannot find -lubsan" in b.stderr or "libasan" in b.stderr and "No such file" in b.stderr):
        pytest.skip("the sanitizer runtimes of g++ are not installed")
    assert b.returncode == 0, b.stderr[-4000:]
    return out


def _run(exe, lines):
    """one answer per case, each a list of floats"""
    text = "".join(ln + "\n" for ln in lines)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1"))
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-1000:], r.stderr[-4000:])
    out = r.stdout.splitlines()
    assert out[-1] == "consensus math: %d cases" % len(lines) and len(out) == len(lines) + 1
    return [[float(t) for t in ln.split()] for ln in out[:-1]]


def _case(cmd, *values):
    return cmd + " " + " ".join(repr(float(v)) for a in values for v in np.asarray(a, dtype=np.float64).reshape(-1))


# ------------------------------------------------------------------------------------------------ the sampler
SEEDS = (0, 1, 0x7FFFFFFF, 0xFFFFFFFF)
# found by search with the checker (ck.sample(seed, h, 7, 7) is None): 64 draws do not collect all of 7 positions.  With S = m = 3 the
# chance of that is 3 (2 / 3)^64 = 2e-11 a hypothesis: no such case exists within reach, the S = 7 ones exercise the same loop.
EXHAUSTED = ((0, 6597, 7), (1, 613, 7), (0x7FFFFFFF, 2958, 7), (0xFFFFFFFF, 1669, 7))


def test_the_sampler_is_the_contracts(exe):
    cases = []
    for S in (7, 3):
        for seed in SEEDS:
            for h in (0, 1, 63, 64, 4095):
                for m in (S - 1, S, S + 1, 8, 64, 1000, 4096):
                    cases.append((S, seed, h, m))
    cases += [(7, seed, h, m) for seed, h, m in EXHAUSTED]
    got = _run(exe, ["sample %d %d %d %d" % c for c in cases])
    failed = 0
    for (S, seed, h, m), g in zip(cases, got):
        want = ck.sample(seed, h, m, S)
        if want is None:
            failed += 1
            assert g[0] == 0, (S, seed, h, m, g)
            # what it holds after a refusal is not specified, beyond being no sample: m < S leaves it all -1
            if m < S:
                assert g[1:] == [-1] * S
        else:
            assert g[0] == 1 and [int(v) for v in g[1:]] == want, (S, seed, h, m, g, want)
            assert len(set(want)) == S and min(want) >= 0 and max(want) < m
    for seed, h, m in EXHAUSTED:
        assert ck.sample(seed, h, m, 7) is None and ck.sample(seed, h, m + 1, 7) is not None
    assert failed == 2 * len(SEEDS) * 5 + len(EXHAUSTED)          # the m = S - 1 cases and the pinned ones, nothing else


def test_the_draw_of_the_checker_on_values_worked_by_hand():
    # seed 0, h 0, k 0: z = 0xBF58476D1CE4E5B9, then the three mixing steps of the header by hand in Python integers
    z = 0xBF58476D1CE4E5B9
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2 ** 64
    z ^= z >> 31
    assert ck.draw(0, 0, 0, 1 << 32) == z >> 32 and ck.draw(0, 0, 0, 1) == 0
    assert all(0 <= ck.draw(s, h, k, 7) < 7 for s in SEEDS for h in (0, 4095) for k in range(64))
    # the seed is the high word, the hypothesis the low one, and the counter starts at 1
    assert ck.draw(1, 0, 0, 1 << 32) != ck.draw(0, 1, 0, 1 << 32) and ck.draw(0, 0, 1, 1 << 32) != ck.draw(0, 0, 0, 1 << 32)
    z = (0x9E3779B97F4A7C15 * (1 << 32) + 2 * 0xBF58476D1CE4E5B9) % 2 ** 64          # seed 1, h 0, k 1
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2 ** 64
    z ^= z >> 31
    assert ck.draw(1, 0, 1, 1000) == ((z >> 32) * 1000) >> 32


# ------------------------------------------------------------------------------------------------ cubic and quartic
def _poly(roots, lead=1.0):
    """c[0] + c[1] x + ... with the given (possibly complex-paired) roots"""
    c = np.poly(roots)
    assert np.abs(np.imag(c)).max() == 0 if np.iscomplexobj(c) else True
    return (np.real(c)[::-1] * lead).astype(np.float64)


def _residual_and_scale(c, x):
    """|p(x)| and sum |c_k| |x|^k, both exactly (rational arithmetic), for the float64 coefficients and the float64 x"""
    xf = Fraction(x)
    p = sum(Fraction(ck_) * xf ** k for k, ck_ in enumerate(c))
    s = sum(abs(Fraction(ck_)) * abs(xf) ** k for k, ck_ in enumerate(c))
    return float(abs(p)), float(s)


# The bound on a simple root's residual.  The returned x is a float64, so at best it is the number nearest the root r: |x - r| <= |x| 2^-53
# and |p(x)| <= |p'(x)| |x| 2^-53 <= degree * S 2^-53 with S = sum |c_k| |x|^k.  The last Newton step moves x by its computed p(x) / p'(x),
# and Horner's p(x) carries an error of at most 2 degree * S 2^-53 (Higham, Accuracy and Stability, section 5.1).  Together
# 3 degree * S 2^-53 = 1.5 degree * S 2^-52; the test allows 2 degree.
def _residual_factor(degree):
    return 2.0 * degree


SIMPLE_CUBICS = [(1e-3, 1.0, 1e3), (-1e3, -1.0, 1e-3), (-2.0, 0.5, 40.0), (1.0, 2.0, 3.0), (-1e-3, 2e-3, 5e-3), (100.0, 300.0, 1000.0), (-7.0, 0.03, 650.0)]
ONE_REAL_CUBICS = [(1e-3, 1 + 2j, 1 - 2j), (-5.0, -0.01 + 100j, -0.01 - 100j), (1e3, 3 + 0.5j, 3 - 0.5j), (0.25, -40 + 1j, -40 - 1j)]
SIMPLE_QUARTICS = [(1e-3, 0.1, 10.0, 1e3), (-3.0, -1.0, 2.0, 5.0), (1.0, 2.0, 3.0, 4.0), (-1e3, -1e-3, 1e-3, 1e3), (0.2, 0.7, 1.9, 4.4), (-60.0, -2.5, 0.004, 12.0)]
TWO_REAL_QUARTICS = [(1.0, 3.0, 2 + 1j, 2 - 1j), (-1e-3, 1e3, 1j, -1j), (0.5, 0.6, -10 + 3j, -10 - 3j)]
NO_REAL_QUARTICS = [(1j, -1j, -1 + 2j, -1 - 2j), (3 + 0.1j, 3 - 0.1j, -3 + 0.1j, -3 - 0.1j), (100j, -100j, 1e-2 + 1e-2j, 1e-2 - 1e-2j)]
# q = 0 in the depressed quartic, given by exact coefficients: x^4 - 5 x^2 + 4 (+-1, +-2), x^4 + 5 x^2 + 4 (none), x^4 - 3 x^2 - 4 (+-2),
# (x - 1)^4 - 5 (x - 1)^2 + 4 = x^4 - 4 x^3 + x^2 + 6 x (-1, 0, 2, 3), x^4 - 16 (+-2)
BIQUADRATICS = [([4.0, 0.0, -5.0, 0.0, 1.0], [-2.0, -1.0, 1.0, 2.0]), ([4.0, 0.0, 5.0, 0.0, 1.0], []), ([-4.0, 0.0, -3.0, 0.0, 1.0], [-2.0, 2.0]),
                ([0.0, 6.0, 1.0, -4.0, 1.0], [-1.0, 0.0, 2.0, 3.0]), ([-16.0, 0.0, 0.0, 0.0, 1.0], [-2.0, 2.0])]
LEADS = (1.0, -0.01, 3.7e3)


def _check_simple(name, c, got, want_real):
    """np.roots agrees with the chosen roots; every real root is returned once; every returned value has a rounding-level residual"""
    degree = len(c) - 1
    ref = np.roots(c[::-1])
    ref_real = np.sort(ref[np.abs(ref.imag) <= 1e-9 * np.maximum(1.0, np.abs(ref.real))].real)
    want_real = np.sort(np.asarray(want_real, dtype=np.float64))
    assert len(ref_real) == len(want_real) and np.allclose(ref_real, want_real, rtol=1e-9, atol=1e-12), (name, ref, want_real)
    count, slots = int(got[0]), np.array(got[1:])
    vals = np.sort(slots[np.isfinite(slots)])
    assert len(slots) == degree and not np.isinf(slots).any() and count == len(vals) == len(want_real), (name, c, got, want_real)
    # the chosen roots lie a factor 1.2 apart at least: within 1e-6 (relative, or of the largest root for a root at 0) identifies each
    assert np.allclose(vals, ref_real, rtol=1e-6, atol=1e-6 * (np.abs(want_real).max() if len(want_real) else 1.0)), (name, vals, ref_real)
    for x in vals:
        res, scale = _residual_and_scale(c, float(x))
        print(name, "root", x, "residual", res, "bound", _residual_factor(degree) * EPS * scale)
        assert res <= _residual_factor(degree) * EPS * scale, (name, c, x, res, scale)


def test_cubic_simple_roots(exe):
    cases = [(r, _poly(r, lead)) for r in SIMPLE_CUBICS + ONE_REAL_CUBICS for lead in LEADS]
    got = _run(exe, [_case("cubic", c) for _, c in cases])
    for (r, c), g in zip(cases, got):
        _check_simple("cubic", c, g, [np.real(x) for x in r if np.imag(x) == 0])


def test_quartic_simple_roots(exe):
    cases = [(r, _poly(r, lead)) for r in SIMPLE_QUARTICS + TWO_REAL_QUARTICS + NO_REAL_QUARTICS for lead in LEADS]
    cases += [(r, np.array(c) * lead) for c, r in BIQUADRATICS for lead in LEADS]
    got = _run(exe, [_case("quartic", c) for _, c in cases])
    for (r, c), g in zip(cases, got):
        _check_simple("quartic", c, g, [np.real(x) for x in r if np.imag(x) == 0])


def test_vanishing_and_non_finite_coefficients_give_no_root(exe):
    nan, inf = float("nan"), float("inf")
    cases = [("cubic", [1.0, 2.0, 3.0, 0.0]), ("cubic", [1.0, 2.0, 3.0, 1e-16]), ("cubic", [-6.0, 11.0, -6.0, -1e-15]), ("cubic", [0.0, 0.0, 0.0, 0.0]),
             ("quartic", [1.0, 2.0, 3.0, 4.0, 0.0]), ("quartic", [1.0, 2.0, 3.0, 4.0, 1e-16]), ("quartic", [24.0, -50.0, 35.0, -10.0, 1e-15]),
             ("quartic", [0.0, 0.0, 0.0, 0.0, 0.0])]
    for bad in (nan, inf, -inf):
        for k in range(4):
            c = [-6.0, 11.0, -6.0, 1.0]
            c[k] = bad
            cases.append(("cubic", c))
        for k in range(5):
            c = [24.0, -50.0, 35.0, -10.0, 1.0]
            c[k] = bad
            cases.append(("quartic", c))
    cases += [("cubic", [nan] * 4), ("quartic", [inf] * 5), ("cubic", [inf, -inf, nan, 1.0])]
    got = _run(exe, [_case(cmd, c) for cmd, c in cases])
    for (cmd, c), g in zip(cases, got):
        assert g[0] == 0 and np.isnan(g[1:]).all() and len(g) == (4 if cmd == "cubic" else 5), (cmd, c, g)


# exactly representable coefficients, so that the roots below ARE the polynomial's
REPEATED = [("cubic", (1.0, 1.0, 3.0)), ("cubic", (2.0, 2.0, 2.0)), ("cubic", (-0.5, -0.5, -0.5)), ("cubic", (-4.0, 0.25, 0.25)), ("cubic", (0.0, 0.0, 5.0)),
            ("cubic", (96.0, 96.0, -1.0)), ("quartic", (1.0, 1.0, 2.0, 3.0)), ("quartic", (1.0, 1.0, 1.0, 2.0)), ("quartic", (2.0, 2.0, 2.0, 2.0)),
            ("quartic", (1.0, 1.0, 3.0, 3.0)), ("quartic", (-0.5, -0.5, 4.0, 8.0)), ("quartic", (0.0, 0.0, -3.0, 3.0)), ("quartic", (-2.0, -2.0, 1j, -1j))]


def test_repeated_roots_stay_finite_and_near(exe):
    """the contract promises nothing about multiplicity: each returned value is finite and within sqrt(eps) scale of a true root (a
    relative change of eps in the coefficients moves a double root by that much; scale: the largest root, 1 at least; factor 4)"""
    cases = [(cmd, r, _poly(r, lead)) for cmd, r in REPEATED for lead in (1.0, -3.0)]
    for cmd, r, c in cases:
        assert all(_residual_and_scale(c, float(np.real(x)))[0] == 0.0 for x in r if np.imag(x) == 0), (cmd, r, c)      # exact roots of the float64 coefficients
    got = _run(exe, [_case(cmd, c) for cmd, _, c in cases])
    for (cmd, r, c), g in zip(cases, got):
        degree = len(c) - 1
        slots = np.array(g[1:])
        vals = slots[~np.isnan(slots)]
        real = np.array([np.real(x) for x in r if np.imag(x) == 0])
        tol = 4.0 * np.sqrt(EPS) * max(1.0, np.abs(real).max())
        print(cmd, r, "returned", vals, "tolerance", tol)
        assert np.isfinite(vals).all() and g[0] == len(vals) <= degree, (cmd, r, g)
        for x in vals:
            assert np.abs(real - x).min() <= tol, (cmd, r, x, tol)


# ------------------------------------------------------------------------------------------------ the 7-point chain
def _exact_views(seed, n):
    """n correspondences of the checker's two views in float64, NOT rounded to float32: they satisfy the true matrix to rounding"""
    rng = np.random.default_rng(seed)
    X = ck._points(rng, n, False)
    x1, _ = ck._project(np.eye(3), np.zeros(3), ck.K, X)
    x2, _ = ck._project(ck.R_VIEW, ck.T_VIEW, ck.K, X)
    return x1, x2


def _seven_case(N, x1, x2):
    return _case("seven", N, np.c_[x1, x2])


def test_seven_point_finds_the_matrix_and_fits_its_points(exe):
    Ft = ck.true_fundamental().reshape(-1)
    cases = []
    for seed in range(12):
        x1, x2 = _exact_views(100 + seed, 40)
        N = ck.hartley_values(x1, x2, np.arange(40))          # the call's normalisation is of ALL usable points, not of the seven
        cases.append((N, x1[:7], x2[:7]))
        cases.append((ck.hartley_values(x1, x2, np.arange(7)), x1[:7], x2[:7]))
    got = _run(exe, [_seven_case(*c) for c in cases])
    for (N, x1, x2), g in zip(cases, got):
        nm = int(g[0])
        assert 1 <= nm <= 3 and len(g) == 1 + 9 * nm, g
        Fs = np.array(g[1:]).reshape(nm, 9)
        for F in Fs:
            assert abs(np.linalg.norm(F) - 1.0) <= 1e-12 and abs(np.linalg.det(F.reshape(3, 3))) <= 1e-9
            fit = float(np.max(ck.error_fundamental(F, x1, x2)))
            assert fit <= 1e-12, (fit, F)                       # px^2: what tests/test_consensus_checker.py asks of the checker's own solver
        near = min(min(np.linalg.norm(F - Ft), np.linalg.norm(F + Ft)) for F in Fs)
        # the number of real solutions is that of the checker's own solver
        sols, roots = ck.seven_point_with_roots(x1, x2)
        print("seven-point: models", nm, "distance of the nearest to the true matrix", near, "checker's solutions", len(sols))
        assert near <= 1e-9, near
        assert ck.close_roots(roots) or len(sols) == nm


def test_seven_point_refuses_degenerate_systems(exe):
    x1, x2 = _exact_views(7, 7)
    N = ck.hartley_values(x1, x2, np.arange(7))
    rep1, rep2 = x1.copy(), x2.copy()
    rep1[4], rep2[4] = rep1[1], rep2[1]                          # a repeated correspondence: rank 6
    t = np.array([0.0, 1.0, 2.5, 4.0, 5.0, 7.5, 9.0])[:, None]
    col1 = np.array([100.0, 80.0]) + t * np.array([32.0, 24.0])  # seven collinear points in either image (exact in float64)
    col2 = np.array([130.0, 60.0]) + t * np.array([32.0, 40.0])
    same = np.tile(x1[:1], (7, 1))
    cases = [(N, rep1, rep2), (ck.hartley_values(col1, col2, np.arange(7)), col1, col2), (N, col1, x2), (N, same, same),
             (np.array([0, 0, 1.0, 0, 0, 1.0]), np.zeros((7, 2)), np.zeros((7, 2)))]
    got = _run(exe, [_seven_case(*c) for c in cases])
    assert [g for g in got] == [[-1.0]] * len(cases), got
    # ... and never a NaN model from non-finite input
    bad = x1.copy()
    bad[2, 0] = np.nan
    worse = x2.copy()
    worse[5, 1] = np.inf
    for g in _run(exe, [_seven_case(N, bad, x2), _seven_case(N, x1, worse), _seven_case(np.full(6, np.nan), x1, x2)]):
        assert g == [-1.0] or g == [0.0], g


# ------------------------------------------------------------------------------------------------ P3P
def _p3p_case(Y):
    """camera-frame points Y (3, 3) of the known pose -> (world points, unit bearings)"""
    Y = np.asarray(Y, dtype=np.float64)
    X = (Y - ck.T_VIEW) @ ck.R_VIEW                               # X = R^T (Y - t)
    J = Y / np.linalg.norm(Y, axis=1)[:, None]
    return X, J


def _triangle(centre, radius, angles, tilt=(0.0, 0.0)):
    """three points at the given angles on a circle about centre, the plane of the circle tilted out of the image plane"""
    out = []
    for a in angles:
        dx, dy = radius * np.cos(a), radius * np.sin(a)
        out.append([centre[0] + dx, centre[1] + dy, centre[2] + tilt[0] * dx + tilt[1] * dy])
    return np.array(out)


P3P_TRIANGLES = {
    "scalene": np.array([[-1.0, 0.5, 6.0], [2.0, -1.0, 9.0], [0.5, 1.5, 5.0]]),
    "isosceles": _triangle((0.7, -0.4, 7.0), 1.5, (0.3, 0.3 + 2.0, 0.3 - 2.0), (0.2, -0.1)),                     # two equal sides in the world
    "isosceles_facing": _triangle((0.05, -0.02, 6.0), 1.0, (np.pi / 2, np.pi / 2 + 2.2, np.pi / 2 - 2.2), (0.05, 0.0)),      # ... nearly facing the camera
    "near_equilateral": _triangle((-0.5, 0.3, 8.0), 2.0, (0.1, 0.1 + 2 * np.pi / 3 + 1e-3, 0.1 - 2 * np.pi / 3 - 2e-3), (0.15, 0.3)),
    "equilateral_tilted": _triangle((1.0, 1.0, 10.0), 2.5, (0.0, 2 * np.pi / 3, -2 * np.pi / 3), (-0.4, 0.25)),
    "on_the_axis": np.array([[0.0, 0.0, 5.0], [1.5, -0.5, 7.0], [-1.0, 2.0, 6.0]]),                                # bearing (0, 0, 1) exactly
    "on_the_axis_isosceles": np.array([[0.0, 0.0, 6.0], [1.0, 0.7, 6.5], [-1.0, 0.9, 6.1]]),
}
# Mirror images of themselves: the apex on the axis of symmetry of the other two, in the world AND in the image.  The mirrored pose then
# coincides with the true one -- a double root of the quartic, where no solver can hold 1e-9 (a double root moves by sqrt(eps) under
# rounding) -- and with the apex as the second point Grunert's u = .../(cos gamma - v cos alpha) is 0 / 0.  Nothing is promised there but
# what holds everywhere: at most four poses, each finite and reproducing the bearings.
P3P_MIRRORED = {
    "facing": _triangle((0.0, 0.0, 6.0), 1.0, (np.pi / 2, np.pi / 2 + 2.2, np.pi / 2 - 2.2)),
    "on_the_axis": np.array([[0.0, 0.0, 6.0], [1.0, 0.7, 6.5], [-1.0, 0.7, 6.5]]),
}


def _check_poses(name, X, J, g):
    """what holds of every answer: the count, finite rotations, the three bearings reproduced at positive depth; the poses (n, 12)"""
    n = int(g[0])
    assert 0 <= n <= 4 and len(g) == 1 + 12 * n, (name, g)
    poses = np.array(g[1:]).reshape(n, 12)
    assert np.isfinite(poses).all()
    for M in poses:
        R, t = M[:9].reshape(3, 3), M[9:]
        assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-9 and np.linalg.det(R) > 0, (name, R)
        Yc = X @ R.T + t
        assert (Yc[:, 2] > 0).all() and (np.einsum("ij,ij->i", Yc, J) > 0).all(), (name, Yc)
        assert np.abs(Yc / np.linalg.norm(Yc, axis=1)[:, None] - J).max() <= 1e-9, (name, Yc, J)
    return poses


@pytest.mark.parametrize("name", sorted(P3P_MIRRORED))
def test_p3p_on_mirror_symmetric_configurations_returns_only_poses_that_fit(exe, name):
    Y = P3P_MIRRORED[name]
    cases = [_p3p_case(Y), _p3p_case(Y[[2, 0, 1]]), _p3p_case(Y[[1, 0, 2]])]
    for (X, J), g in zip(cases, _run(exe, [_case("p3p", X, J) for X, J in cases])):
        print(name, "poses", len(_check_poses(name, X, J, g)))


@pytest.mark.parametrize("name", sorted(P3P_TRIANGLES))
def test_p3p_finds_the_pose_and_every_pose_reproduces_the_bearings(exe, name):
    Y = P3P_TRIANGLES[name]
    cases = [_p3p_case(Y), _p3p_case(Y[[2, 0, 1]]), _p3p_case(Y[[1, 0, 2]])]
    got = _run(exe, [_case("p3p", X, J) for X, J in cases])
    for (X, J), g in zip(cases, got):
        poses = _check_poses(name, X, J, g)
        assert len(poses) >= 1, (name, g)
        best = min(max(np.abs(M[:9].reshape(3, 3) - ck.R_VIEW).max(), np.abs(M[9:] - ck.T_VIEW).max()) for M in poses)
        print(name, "poses", len(poses), "distance of the nearest to the true pose", best)
        assert best <= 1e-9, (name, best, poses)


def test_p3p_refuses_collinear_and_repeated_world_points(exe):
    X, J = _p3p_case(P3P_TRIANGLES["scalene"])
    line = np.array([[0.0, 0.0, 5.0], [1.0, 0.5, 6.0], [3.0, 1.5, 8.0]])           # collinear in the world (exactly), bearings of a real view
    cases = [(line, J), (np.array([X[0], X[0], X[2]]), J), (np.array([X[0], X[1], X[0]]), J), (np.array([X[0], X[0], X[0]]), J),
             (X, np.array([J[0], J[0], J[2]])),                                        # repeated bearings
             _p3p_case(np.array([[0.0, 0.0, 5.0], [1.0, 0.5, 6.0], [3.0, 1.5, 8.0]]))]     # collinear in the world and hence in the image
    got = _run(exe, [_case("p3p", A, B) for A, B in cases])
    assert got == [[0.0]] * len(cases), got
    nanX = X.copy()
    nanX[1, 2] = np.nan
    for g in _run(exe, [_case("p3p", nanX, J), _case("p3p", X, np.full((3, 3), np.nan))]):
        assert g == [0.0], g
