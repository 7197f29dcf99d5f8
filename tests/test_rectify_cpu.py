"""CPU: the restatement of the raw-stereo input path in tests/rectify_ref.py against hand-derived answers."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rectify_ref as R   # noqa: E402

I3 = np.eye(3)


def test_identity_map_is_the_pixel_grid():
    mx, my = R.init_rectify_map(I3, [0, 0, 0, 0], I3, I3, 37, 23)
    y, x = np.mgrid[0:23, 0:37]
    assert (mx == x).all() and (my == y).all()
    assert mx.dtype == np.float32 and my.dtype == np.float32


@pytest.mark.parametrize("c", [0.5, 2.25, -3.75, 16.0])
def test_dyadic_principal_point_shift_is_exact(c):
    P = np.eye(3)
    P[0, 2] = c
    P[1, 2] = -c
    mx, my = R.init_rectify_map(I3, [0, 0, 0, 0, 0], I3, P, 40, 12)
    y, x = np.mgrid[0:12, 0:40]
    assert (mx == (x - c).astype(np.float32)).all() and (my == (y + c).astype(np.float32)).all()


def test_row_recurrence_is_sequential():
    # K = I, R = I, D = 0, P = diag(10, 1, 1): ir[0] = 0.1, ir[2] = 0, w = 1, so the float64 u is _x itself.  0.1 is not dyadic:
    # the sequential sum and j * 0.1 differ in the last bits along the row (the float32 cast hides it, so compare before the cast)
    P = np.diag([10.0, 1.0, 1.0])
    u, _ = R.init_rectify_map(I3, [0, 0, 0, 0], I3, P, 4000, 1, f64=True)
    step = np.float64(1.0) / np.float64(10.0)
    seq, acc = [], np.float64(0.0)
    for _ in range(4000):   # OpenCV's loop: for (j = 0; j < w; j++, _x += ir[0])
        seq.append(acc)
        acc = acc + step
    assert (u[0] == np.array(seq)).all()
    mul = np.arange(4000, dtype=np.float64) * step
    assert (u[0] != mul).sum() > 1000
    mx, _ = R.init_rectify_map(I3, [0, 0, 0, 0], I3, P, 4000, 1)
    assert (mx[0] == np.array(seq).astype(np.float32)).all()


def test_rounding_of_map_values_is_half_to_even():
    m = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5], np.float64) / 32
    assert list(R.cv_round_q5(m.astype(np.float32))) == [0, 2, 2, 0, -2, -2]


def test_negative_coordinates_shift_arithmetically():
    sx, sy, ax, ay = R.fixed_maps(np.float32([-0.25]), np.float32([-0.25]))
    assert (sx[0], ax[0], sy[0], ay[0]) == (-1, 24, -1, 24)


def test_nan_and_inf_map_to_int_min_and_read_zero():
    m = np.float32([np.nan, np.inf, -np.inf, 3e9, -3e9])
    assert (R.cv_round_q5(m) == R.INT_MIN).all()
    sx, _, ax, _ = R.fixed_maps(m, np.zeros(5, np.float32))
    assert (sx == -32768).all() and (ax == 0).all()
    src = np.full((4, 4), 255, np.uint8)
    out = R.remap(src, np.float32([[np.nan, 1.0]]), np.float32([[1.0, np.inf]]))
    assert out.tolist() == [[0, 0]]


def test_right_and_bottom_edge_taps_read_zero():
    src = np.full((3, 5), 200, np.uint8)
    # x = 4.5 on the last column: half of the right tap is outside; y = 2.5 likewise at the bottom
    out = R.remap(src, np.float32([[4.5, 1.0, 4.5]]), np.float32([[1.0, 2.5, 2.5]]))
    assert out.tolist() == [[100, 100, 50]]
    # a map value exactly on the last pixel reads it fully
    assert R.remap(src, np.float32([[4.0]]), np.float32([[2.0]])).tolist() == [[200]]


def test_q15_integral_entry_equals_the_q10_form_for_all_pairs():
    # remap's table may store the integral entry (ax = ay = 0) as {32767, 0, 0, 1}: saturate_cast<short>(32768) plus the sum
    # correction that moves the lost unit to the largest other weight
    p = np.arange(256, dtype=np.int64)
    p00, p11 = np.meshgrid(p, p, indexing="ij")
    zero = np.zeros_like(p00)
    got = R.bilinear_q15([p00, zero, zero, p11], [32767, 0, 0, 1])
    want = R.bilinear_q10(p00, zero, zero, p11, 0, 0)
    assert (got == want).all() and (want == p00).all()


def test_q15_table_equals_the_q10_form():
    rng = np.random.default_rng(3)
    p = rng.integers(0, 256, (4, 20000))
    ax, ay = rng.integers(0, 32, 20000), rng.integers(0, 32, 20000)
    w = [32 * (32 - ay) * (32 - ax), 32 * (32 - ay) * ax, 32 * ay * (32 - ax), 32 * ay * ax]
    assert (R.bilinear_q15(p, w) == R.bilinear_q10(p[0], p[1], p[2], p[3], ax, ay)).all()
    assert ((32 - ax) * 255 + ax * 255).max() <= 8160


def test_remap_then_gray_differs_from_gray_then_remap():
    # two pixels of complementary colours, sampled half way: each channel rounds on its own before the conversion
    src = np.array([[[255, 0, 1], [0, 255, 0]]], np.uint8)
    mx, my = np.float32([[0.5]]), np.float32([[0.0]])
    a = R.rectify_gray(src, mx, my, rgb=True)
    b = R.remap(R.gray_from_color(src, rgb=True), mx, my)
    assert a.shape == b.shape == (1, 1) and a[0, 0] != b[0, 0]


def test_inverse_exact_on_diagonal_powers_of_two():
    m = np.diag([4.0, 0.5, 2.0 ** -10])
    assert (R.invert3(m) == np.diag([0.25, 2.0, 2.0 ** 10]).ravel()).all()


def test_inverse_agrees_with_numpy():
    rng = np.random.default_rng(5)
    for _ in range(200):   # well-conditioned matrices of camera-like scales
        m = (rng.normal(size=(3, 3)) + 4 * np.eye(3)) * 10 ** rng.uniform(-2, 3)
        t = R.invert3(m).reshape(3, 3)
        ref = np.linalg.inv(m)
        assert np.abs(t - ref).max() <= 1e-12 * np.abs(ref).max()


def test_singular_matrix_has_no_inverse():
    assert R.invert3(np.ones((3, 3))) is None
    with pytest.raises(ValueError):
        R.init_rectify_map(I3, [0, 0, 0, 0], np.zeros((3, 3)), I3, 4, 4)


@pytest.mark.parametrize("n", [0, 1, 3, 6, 7, 12, 14])
def test_other_coefficient_counts_are_rejected(n):
    with pytest.raises(ValueError):
        R.init_rectify_map(I3, np.zeros(n), I3, I3, 4, 4)


def test_euroc_maps_stay_in_the_image_and_shift_with_distortion():
    L = R.EUROC_L
    mx, my = R.init_rectify_map(L["K"], L["D"], L["R"], L["P"], *R.EUROC_SIZE)
    assert np.isfinite(mx).all() and np.isfinite(my).all()
    # the centre of the rectified image comes from near the raw principal point; the barrel lens pulls the corners inwards
    assert abs(mx[252, 367] - 367.2) < 6 and abs(my[252, 367] - 248.4) < 6
    assert mx[0, 0] > 0 and my[0, 0] > 0
