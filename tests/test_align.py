"""Alignment (K7) + blur quality (K8): FaceAligner.align / FaceQualityFilter (face_recognition.py:50-158).

PARITY UNPINNED against OpenCV (absent here; the reference has no aligned-crop
fixtures).  The HIP kernels are pinned bit for bit to oracle/align_ref.py, the
restatement of OpenCV's uint8 fixed-point arithmetic; CPU tests check the
restatement's own invariants (identity / integer shifts copy pixels exactly,
half-pixel shifts round half up, the fit recovers an exact similarity, the
RANSAC consensus drops outliers, cv::RNG's sequence and the adaptive iteration
count follow OpenCV's published formulas).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import align_ref as A


def _faces(rng, n, H, W, S=112, jitter=2.0, scale=(1.0, 3.0)):
    """n landmark sets: the reference template scaled/rotated/translated into the frame + noise."""
    t = A.reference_template(S).astype(np.float64)
    out = []
    for _ in range(n):
        s = rng.uniform(*scale)
        th = rng.uniform(-0.4, 0.4)
        R = s * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        c = np.array([rng.uniform(-50, W + 50), rng.uniform(-50, H + 50)])  # some faces cross the border
        p = (t - S / 2) @ R.T + c + rng.normal(0, jitter, t.shape)
        out.append(p)
    return np.array(out, dtype=np.float32)


# ---------------------------------------------------------------- CPU: the restatement
def test_warp_identity_and_integer_shift_copy_pixels():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (40, 50, 3), dtype=np.uint8)
    I = np.array([[1.0, 0, 0], [0, 1.0, 0]])
    assert np.array_equal(A.warp_affine_linear(img, I, 32), img[:32, :32])
    T = np.array([[1.0, 0, -3], [0, 1.0, -5]])  # dst(x,y) = src(x+3, y+5)
    assert np.array_equal(A.warp_affine_linear(img, T, 30), img[5:35, 3:33])
    out = A.warp_affine_linear(img, np.array([[1.0, 0, 10], [0, 1.0, 10]]), 20)
    assert (out[:10] == 0).all() and (out[:, :10] == 0).all()  # BORDER_CONSTANT 0


def test_warp_half_pixel_rounds_half_up():
    img = np.zeros((4, 8, 1), np.uint8)
    img[0, :, 0] = [10, 11, 20, 30, 40, 50, 60, 70]
    M = np.array([[1.0, 0, -0.5], [0, 1.0, 0]])  # dst(x) = src(x + 0.5)
    out = A.warp_affine_linear(img, M, 4)[0, :, 0]
    assert out.tolist() == [11, 16, 25, 35]  # (10+11+1)//2, (11+20+1)//2, ...


def test_similarity_fit_recovers_exact_similarity():
    t = A.reference_template(112)
    M = np.array([[0.8, -0.3, 12.5], [0.3, 0.8, -7.25]])
    src = ((t.astype(np.float64) - M[:, 2]) @ np.linalg.inv(M[:, :2]).T).astype(np.float32)
    got = A.fit_similarity(src, t)
    assert np.abs(got - M).max() < 1e-4


def test_fit_outlier_is_excluded():
    t = A.reference_template(112).astype(np.float64)
    src = t * 2.0 + 10
    src[2] += 40.0  # nose far off: RANSAC drops it
    M = A.fit_similarity(src.astype(np.float32), t.astype(np.float32))
    assert np.abs(M - np.array([[0.5, 0, -5], [0, 0.5, -5]])).max() < 1e-9


def test_cv_rng_sequence():
    """cv::RNG((uint64)-1) as RANSAC seeds it: state' = lo32(state) * 4164903690 + hi32(state)."""
    r = A.CvRNG((1 << 64) - 1)
    s = (1 << 64) - 1
    for _ in range(5):
        s = ((s & 0xFFFFFFFF) * 4164903690 + (s >> 32)) & ((1 << 64) - 1)
        assert r.next() == s & 0xFFFFFFFF
    assert A.CvRNG(0).state == 0xFFFFFFFF  # RNG(0) is seeded with 0xffffffff
    assert [A.CvRNG((1 << 64) - 1).uniform(3, 3)] == [3]


def test_ransac_iteration_update():
    """RANSACUpdateNumIters: log(1-p)/log(1-(1-ep)^2), capped; every inlier found -> 0 more iterations."""
    assert A._update_num_iters(0.99, 0.0, 2, 2000) == 0
    want = int(round(np.log(1 - 0.99) / np.log(1 - 0.6 ** 2)))
    assert A._update_num_iters(0.99, 0.4, 2, 2000) == want == 10
    assert A._update_num_iters(0.99, 0.4, 2, 5) == 5


def _hard_landmarks(rng, n, S=112):
    """Landmark sets whose least-squares similarity leaves a residual > 3 px (outliers / strong noise)."""
    t = A.reference_template(S).astype(np.float64)
    out = []
    while len(out) < n:
        s = rng.uniform(1.0, 4.0)
        th = rng.uniform(-0.5, 0.5)
        R = s * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        p = (t - S / 2) @ R.T + rng.uniform(100, 1800, 2) + rng.normal(0, rng.uniform(1, 6), t.shape)
        k = rng.integers(0, 3)
        p[rng.choice(5, k, replace=False)] += rng.normal(0, 25, (k, 2))  # 0-2 gross outliers
        p = p.astype(np.float32)
        q = p.astype(np.float64)
        one, zero = np.ones((5, 1)), np.zeros((5, 1))
        lhs = np.block([[q[:, :1], -q[:, 1:], one, zero], [q[:, 1:], q[:, :1], zero, one]])
        a, b, tx, ty = np.linalg.lstsq(lhs, np.concatenate([t[:, 0], t[:, 1]]), rcond=None)[0]
        res = np.hypot(a * p[:, 0] - b * p[:, 1] + tx - t[:, 0], b * p[:, 0] + a * p[:, 1] + ty - t[:, 1])
        if res.max() > 3.0:
            out.append(p)
    return np.array(out, dtype=np.float32)


def test_host_fit_matches_restatement_bitwise():
    """The C++ fit behind fr_align_faces performs the oracle's IEEE operation sequence (no GPU needed):
    ordinary landmark sets and sets whose least-squares residuals exceed the 3-px RANSAC threshold."""
    from facerecognitionpipeline_amd import _lib
    lib = _lib.load()
    lib.frt_fit_similarity.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int, ctypes.c_void_p]
    rng = np.random.default_rng(1)
    t = A.reference_template(112)
    sets = list(_faces(rng, 40, 1080, 1920, jitter=3.0)) + list(_hard_landmarks(rng, 60))
    partial = 0
    for lm in sets:
        M = np.zeros(6)
        assert lib.frt_fit_similarity(lm.ctypes.data, t.ctypes.data, 5, M.ctypes.data) == 0
        want = A.fit_similarity(lm, t)
        assert np.array_equal(M.reshape(2, 3), want)
        e = lm.astype(np.float64) @ want[:, :2].T + want[:, 2] - t
        partial += int((np.hypot(e[:, 0], e[:, 1]) > 3.0).any())
    assert partial >= 10  # the hard sets really exercise the consensus (some points left out)


def test_laplacian_var_matches_direct_definition():
    rng = np.random.default_rng(2)
    g = rng.integers(0, 256, (112, 112), dtype=np.uint8)
    gi = g.astype(np.int64)
    P = np.pad(gi, 1, mode="reflect")
    L = P[:-2, 1:-1] + P[2:, 1:-1] + P[1:-1, :-2] + P[1:-1, 2:] - 4 * gi
    n = L.size
    exact = (n * (L * L).sum() - L.sum() ** 2) / n ** 2
    assert abs(A.laplacian_var(g) - exact) <= 1e-12 * exact


def test_pose_angles_of_frontal_template():
    p = A.pose_angles(A.reference_template(112).astype(np.float64))
    assert abs(p["roll"]) < 1e-4 and abs(p["yaw"]) < 1e-4  # float32 template coordinates
    assert abs(p["pitch"] - ((0.61 - 0.46) / (0.74 - 0.46) - 0.5) * 60) < 1e-4


def test_warp_of_a_plane_stays_within_the_fixed_point_error_bound():
    """On the plane 2x + 3y the bilinear sample is exact, so an interior pixel of the restatement
    differs from the exact affine sample only by its own roundings: 0.5 of the output, and per axis
    1/64 px of the 1/32-px position plus 1/1024 px of the two cvRounds, times the slopes 2 + 3:
    0.5 + (1/64 + 1/1024) * 5 = 0.583 (worst seen: 0.580)."""
    H, W, S = 40, 50, 32
    yy, xx = np.mgrid[:H, :W]
    img = (2 * xx + 3 * yy).astype(np.uint8)[..., None]
    assert img.max() == 2 * (W - 1) + 3 * (H - 1) <= 255
    bound = 0.5 + (1 / 64 + 1 / 1024) * (2 + 3)
    rng = np.random.default_rng(2024)
    oy, ox = np.mgrid[:S, :S]
    worst, n_int = 0.0, 0
    for _ in range(200):
        s, th = rng.uniform(0.5, 2.0), rng.uniform(-np.pi, np.pi)
        c = np.array([rng.uniform(10, W - 10), rng.uniform(10, H - 10)])
        L = s * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        Mi = np.concatenate([L, (c - L @ np.array([S / 2, S / 2]))[:, None]], axis=1)  # output centre -> c
        M = A.invert_affine(Mi)
        Mb = A.invert_affine(M)
        px = Mb[0, 0] * ox + Mb[0, 1] * oy + Mb[0, 2]
        py = Mb[1, 0] * ox + Mb[1, 1] * oy + Mb[1, 2]
        X, Y = A.warp_maps(M, S)
        sx, sy = X >> 5, Y >> 5
        inside = (sx >= 0) & (sx + 1 < W) & (sy >= 0) & (sy + 1 < H)
        got = A.warp_affine_linear(img, M, S)[..., 0].astype(np.float64)
        err = np.abs(got - (2 * px + 3 * py))[inside]
        n_int += int(inside.sum())
        if err.size:
            worst = max(worst, float(err.max()))
    assert n_int > 200 * S * S // 4
    assert worst <= bound, worst


def test_far_translation_is_all_border_in_the_restatement():
    """What the warp kernels are held to far outside the 32-bit range: the restatement keeps 64-bit
    positions, so every tap is outside and the crop is the border value."""
    img = np.random.default_rng(3).integers(1, 256, (5, 7, 3), dtype=np.uint8)
    M = np.array([[1.0, 0, -(2 ** 32 + 5)], [0, 1.0, 0]])
    X, Y = A.warp_maps(M, 17)
    assert (X >> 5).min() >= 2 ** 32 and ((X >> 5).astype(np.int32) < 7).any()  # narrowed, it lands in the frame
    assert (Y >> 5).tolist() == [[y] * 17 for y in range(17)]
    assert not A.warp_affine_linear(img, M, 17).any()


def test_letterbox_widths_cover_every_tail_of_the_simd_split():
    """Portrait sources 128 x w, w = 1..16, letterbox to new_w = 5w: every residue of new_w mod 16 and
    of the row's bytes mod 4.  The host's resize_simd_end must split each such row where the
    restatement's loop (oracle/scrfd.py resize_linear_u8) does."""
    from oracle import scrfd as R
    from tests import _frt
    tails = {}
    for w in range(1, 17):
        new_w, new_h, _ = R.letterbox_geometry(128, w)
        assert (new_w, new_h) == (5 * w, 640)
        row = new_w * 3
        x = 0
        while x <= row - 16:
            x += 16
        while x < row - 8:
            x += 8
        assert _frt.resize_simd_end(row) == x
        assert 0 <= row - x <= 15 and (row - x <= 8 or x == 0)  # a scalar tail of at most 8 bytes (15: no SIMD part)
        tails[new_w % 16] = row - x
    assert sorted(tails) == list(range(16)) and {5 * w * 3 % 4 for w in range(1, 17)} == {0, 1, 2, 3}
    assert len(set(tails.values())) >= 8


# ---------------------------------------------------------------- GPU: kernels vs restatement
@pytest.mark.gpu
@pytest.mark.parametrize("S,n", [(112, 24), (224, 24), (112, 60)])  # n > 48: maps via device memory
def test_align_kernel_bit_exact(S, n):
    from facerecognitionpipeline_amd.face_recognition import FaceAligner
    rng = np.random.default_rng(10 + S + n)
    H, W = 1080, 1920
    frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    lms = _faces(rng, n, H, W, S=S)
    al = FaceAligner(output_size=S, device="cuda:0")
    got = al.align_batch(torch.from_numpy(frame).cuda(), lms).cpu().numpy()
    t = A.reference_template(S)
    for i, lm in enumerate(lms):
        ref = A.warp_affine_linear(frame, A.fit_similarity(lm, t), S)
        assert np.array_equal(got[i], ref), f"face {i}: {np.count_nonzero(got[i] != ref)} px differ"
    one = al.align(frame, lms[0])                      # reference host signature
    assert one.dtype == np.uint8 and np.array_equal(one, got[0])
    aff = al.align_batch(torch.from_numpy(frame).cuda(), lms[:3], method="affine").cpu().numpy()
    from facerecognitionpipeline_amd.face_recognition import affine_from_3_points
    for i in range(3):
        assert np.array_equal(aff[i], A.warp_affine_linear(frame, affine_from_3_points(lms[i][:3], t[:3]), S))


# blur_kernel restates numpy's float64 summation order as derived from numpy 2.2 (the build
# image's 2.2.6): bitwise there; another numpy release may buffer its reduction differently, so
# elsewhere the device value is held to a relative tolerance instead
NUMPY_ORDER_PINNED = np.__version__.startswith("2.2.")


def _blur_equal(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if NUMPY_ORDER_PINNED:
        return np.array_equal(got, ref)
    return np.allclose(got, ref, rtol=1e-12, atol=0.0)


@pytest.mark.gpu
def test_blur_kernel_matches_restatement():
    from facerecognitionpipeline_amd.face_recognition import FaceQualityFilter
    rng = np.random.default_rng(20)
    crops = rng.integers(0, 256, (9, 112, 112, 3), dtype=np.uint8)
    crops[1] = 128                                    # flat crop: variance 0
    crops[2] = crops[2] // 16 * 16
    qf = FaceQualityFilter()
    got = qf.compute_blur_scores(crops)
    ref = np.array([A.blur_score(c) for c in crops])
    # bitwise numpy's ndarray.var() (its chunked pairwise summation order), as the reference gets it
    assert _blur_equal(got, ref)
    assert got[1] == 0.0
    big = rng.integers(0, 256, (2, 224, 224, 3), dtype=np.uint8)
    assert _blur_equal(qf.compute_blur_scores(big), [A.blur_score(c) for c in big])
    # smooth crops (small variances, many equal Laplacians) and odd sizes: chunk and leaf edges;
    # up to 320 (13 chunks, 155,576 bytes of LDS) one block per image, 448 (25 chunks) the
    # multi-block form; the limit between the two forms: test_blur_at_the_one_block_limit
    for S in (7, 8, 9, 90, 91, 129, 200, 256, 320, 448):
        yy, xx = np.mgrid[0:S, 0:S]
        sm = np.stack([(yy * 3 + xx) % 256, (xx * 2) % 256, (yy + 40) % 256], -1).astype(np.uint8)[None]
        sm = np.concatenate([sm, rng.integers(0, 256, (1, S, S, 3), dtype=np.uint8)])
        assert _blur_equal(qf.compute_blur_scores(sm), [A.blur_score(c) for c in sm]), S


@pytest.mark.gpu
def test_blur_any_shape_gray_and_rgba():
    """compute_blur_score takes what cv2.Laplacian(gray, CV_64F).var() takes (face_recognition.py:94-99):
    a 2-D gray image or an RGB one, any height x width, never refused."""
    import torch
    from facerecognitionpipeline_amd.face_recognition import FaceQualityFilter
    rng = np.random.default_rng(21)
    qf = FaceQualityFilter()
    for (H, W) in ((1, 1), (1, 9), (9, 1), (2, 2), (3, 5), (112, 96), (97, 300), (480, 640), (1080, 7)):
        rgb = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
        gray = rng.integers(0, 256, (2, H, W), dtype=np.uint8)
        assert _blur_equal(qf.compute_blur_scores(rgb), [A.blur_score(c) for c in rgb]), (H, W)
        assert _blur_equal(qf.compute_blur_scores(gray), [A.laplacian_var(g) for g in gray]), (H, W)
        # the single-image reference signature: 3-D RGB, 2-D gray; np.float64 like ndarray.var()
        one = qf.compute_blur_score(gray[0])
        assert type(one) is np.float64 and _blur_equal([one], [A.laplacian_var(gray[0])])
        assert _blur_equal([qf.compute_blur_score(rgb[1])], [A.blur_score(rgb[1])])
        # an RGBA image: cvtColor(RGB2GRAY) ignores alpha
        rgba = np.concatenate([rgb, rng.integers(0, 256, (2, H, W, 1), dtype=np.uint8)], axis=3)
        assert _blur_equal(qf.compute_blur_scores(rgba), [A.blur_score(c) for c in rgb]), (H, W)
    # the gray form of an RGB crop is the RGB crop's score (RGB2GRAY is what the kernel applies)
    rgb = rng.integers(0, 256, (3, 320, 200, 3), dtype=np.uint8)
    g = np.stack([A.rgb_to_gray(c) for c in rgb])
    assert np.array_equal(qf.compute_blur_scores(g), qf.compute_blur_scores(rgb))
    # device tensors in, same values
    assert np.array_equal(qf.compute_blur_scores(torch.from_numpy(g).cuda()), qf.compute_blur_scores(g))
    # an empty batch is an empty result; a wrong rank is refused
    assert qf.compute_blur_scores(np.zeros((0, 8, 8, 3), np.uint8)).shape == (0,)
    with pytest.raises(ValueError):
        qf.compute_blur_scores(np.zeros((8, 8), np.uint8))


# blur_kernel (one block per image) keeps everything in LDS: 32 bytes of int64 wave sums, per chunk of
# 8192 pixels 2 * 128 float64 values and 2 * 255 int32 node ranges (4088 bytes), and one gray byte per
# pixel: 32 + 4088 * ceil(n / 8192) + n bytes for n pixels, all of it dynamic.  A gfx950 workgroup has
# 160 KiB = 163,840 bytes.  13 chunks (n <= 106,496) need at most 159,672; with 14 chunks
# 32 + 57,232 + n <= 163,840 holds up to n = 106,576.  So 106,576 pixels is the largest one-block
# image and 106,577 the smallest that takes the three-launch form.  (Before the wave sums were counted
# the launcher drew the line at 106,608 and asked for up to 163,872 bytes in between.)
ONE_BLOCK_MAX_PIXELS = 106_576
BLUR_SEAM_SHAPES = [
    (256, 416),    # 106,496: 13 full chunks
    (16, 6661),    # 106,576: the last one-block count
    (197, 541),    # 106,577: the first multi-block count
    (323, 330),    # 106,590  \
    (325, 328),    # 106,600   > counts the launcher once sent to one block with too much LDS
    (17, 6271),    # 106,607  /
    (48, 2221),    # 106,608: the last of them
    (181, 589),    # 106,609: multi-block before and after
]


@functools.lru_cache(maxsize=None)
def _blur_seam_case(H, W):
    """Two RGBA images of H x W, one smooth and one random, and the reference scores of their RGB and
    gray forms (computed once for the three channel counts; the arrays are never changed)."""
    rng = np.random.default_rng(H * 10007 + W)
    yy, xx = np.mgrid[0:H, 0:W]
    smooth = np.stack([(yy * 3 + xx) % 256, (xx * 2) % 256, (yy + 40) % 256, (xx + yy) % 256], -1).astype(np.uint8)
    rgba = np.stack([smooth, rng.integers(0, 256, (H, W, 4), dtype=np.uint8)])
    gray = np.ascontiguousarray(rgba[..., 1])
    ref_rgb = np.array([A.blur_score(c[..., :3]) for c in rgba])
    ref_gray = np.array([A.laplacian_var(g) for g in gray])
    for a in (rgba, gray, ref_rgb, ref_gray):
        a.setflags(write=False)
    return rgba, gray, ref_rgb, ref_gray


@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("H,W", BLUR_SEAM_SHAPES)
def test_blur_across_the_one_block_limit(H, W, C):
    """Pixel counts around the largest image blur_kernel's LDS holds, gray, RGB and RGBA: whichever
    form the launcher picks returns numpy's bits, and never asks for more LDS than a workgroup has."""
    from facerecognitionpipeline_amd.face_recognition import FaceQualityFilter
    rgba, gray, ref_rgb, ref_gray = _blur_seam_case(H, W)
    qf = FaceQualityFilter()
    if C == 1:
        assert _blur_equal(qf.compute_blur_scores(gray.copy()), ref_gray)
    else:
        assert _blur_equal(qf.compute_blur_scores(rgba[..., :C].copy()), ref_rgb)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,over", [(4, 26644, 0), (541, 197, 1)], ids=["last_one_block", "first_multi_block"])
def test_blur_at_the_one_block_limit(H, W, over):
    """One image on each side of ONE_BLOCK_MAX_PIXELS, in other shapes than the table's (long rows;
    tall and narrow), a batch of 3 so the multi-block form's per-image workspace slices matter."""
    from facerecognitionpipeline_amd.face_recognition import FaceQualityFilter
    assert H * W == ONE_BLOCK_MAX_PIXELS + over
    rng = np.random.default_rng(H)
    rgb = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    rgb[1] = rgb[1] // 32 * 32
    assert _blur_equal(FaceQualityFilter().compute_blur_scores(rgb), [A.blur_score(c) for c in rgb])


@pytest.mark.gpu
def test_processor_large_output_size_and_gray_aligner():
    """FaceProcessor(output_size=320): the reference blur-scores crops of any size; FaceAligner on a
    2-D gray frame returns the 2-D crop, like cv2.warpAffine."""
    from facerecognitionpipeline_amd.face_recognition import FaceAligner, FaceQualityFilter
    rng = np.random.default_rng(22)
    frame = rng.integers(0, 256, (400, 500, 3), dtype=np.uint8)
    t = A.reference_template(320)
    lm = (t - 160) * 0.9 + np.array([250.0, 200.0])
    al = FaceAligner(output_size=320)
    crop = al.align(frame, lm.astype(np.float32))
    want = A.warp_affine_linear(frame, A.fit_similarity(lm.astype(np.float32), t), 320)
    assert np.array_equal(crop, want)
    qf = FaceQualityFilter()
    assert _blur_equal([qf.compute_blur_score(crop)], [A.blur_score(want)])
    gray = frame[..., 1].copy()
    g = al.align(gray, lm.astype(np.float32))
    assert g.ndim == 2 and np.array_equal(g, A.warp_affine_linear(gray[..., None], A.fit_similarity(
        lm.astype(np.float32), t), 320)[..., 0])
    assert _blur_equal([qf.compute_blur_score(g)], [A.laplacian_var(g)])


@pytest.mark.gpu
def test_processor_align_embed_match_stays_on_device():
    """frame -> device align -> embed == host-aligned crops -> embed; FaceProcessor filter/sort semantics."""
    from facerecognitionpipeline_amd.face_embedder import FaceEmbedder
    from facerecognitionpipeline_amd.face_recognition import FaceAligner, FaceProcessor
    rng = np.random.default_rng(30)
    H, W = 720, 1280
    frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    lms = _faces(rng, 6, H, W, S=112, scale=(1.5, 2.5))
    emb = FaceEmbedder(architecture="ir_50", model_path="synthetic", max_batch=16)
    al = FaceAligner(112)
    crops_dev = al.align_batch(torch.from_numpy(frame).cuda(), lms)
    e_dev = emb.embed_tensor(crops_dev).cpu().numpy()
    t = A.reference_template(112)
    host = [A.warp_affine_linear(frame, A.fit_similarity(lm, t), 112) for lm in lms]
    assert np.array_equal(e_dev, emb.extract_embeddings_batch(host))

    class FakeDetector:
        def detect(self, image):
            return [{"bbox": np.array([0, 0, 200, 200], np.int32), "landmarks": lm, "det_score": 0.9 - 0.01 * i}
                    for i, lm in enumerate(lms)]

    fp = FaceProcessor(output_size=112, detector=FakeDetector(),
                       quality_filter_config={"max_yaw": 90, "max_pitch": 90, "max_roll": 90, "blur_threshold": 0})
    out = fp.process_numpy(frame, return_all=True)
    assert len(out) == 6
    keys = [r["det_score"] * r["quality_metrics"]["blur_score"] for r in out]
    assert keys == sorted(keys, reverse=True)
    best = fp.process_numpy(frame)
    assert len(best) == 1 and np.array_equal(best[0]["aligned_face"], out[0]["aligned_face"])
    # grayscale frame: the reference warps the 2-D frame and blur-scores the 2-D crop
    gray = A.rgb_to_gray(frame)
    g_out = fp.process_numpy(gray, return_all=True)
    assert len(g_out) == 6
    for r in g_out:
        assert r["aligned_face"].ndim == 2
        i = [j for j, lm in enumerate(lms) if np.array_equal(lm, r["landmarks"])][0]
        want = A.warp_affine_linear(gray[:, :, None], A.fit_similarity(lms[i], t), 112)[:, :, 0]
        assert np.array_equal(r["aligned_face"], want)
        assert r["quality_metrics"]["blur_score"] == A.laplacian_var(want)


@pytest.mark.gpu
def test_recognition_pipeline_frame_to_matches(tmp_path):
    """frame + detections -> device align -> blur/quality gate -> batched embed+match (serving path)."""
    from facerecognitionpipeline_amd.face_embedder import FaceEmbedder
    from facerecognitionpipeline_amd.gallery_manager import GalleryManager
    from facerecognitionpipeline_amd.pipeline import RecognitionPipeline
    rng = np.random.default_rng(40)
    H, W = 1080, 1920
    frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    lms = _faces(rng, 8, H - 200, W - 200, S=112, scale=(1.5, 2.0)) + 100  # inside the frame
    emb = FaceEmbedder(architecture="ir_50", model_path="synthetic", max_batch=16)
    t = A.reference_template(112)
    crops = np.stack([A.warp_affine_linear(frame, A.fit_similarity(lm, t), 112) for lm in lms])
    gm = GalleryManager(gallery_path=str(tmp_path / "g" / "s.npz"), device=emb.device, verbose=False)
    for i, e in enumerate(emb.extract_embeddings_batch(list(crops))):
        gm.add_student(f"S{i}", f"N{i}", e)
    dets = [{"bbox": np.array([0, 0, 150, 150], np.int32), "landmarks": lm, "det_score": 0.9} for lm in lms]
    dets[3]["det_score"] = 0.1                                       # fails the det-score gate
    pipe = RecognitionPipeline(emb, gm, {"max_yaw": 90, "max_pitch": 90, "max_roll": 90, "blur_threshold": 0})
    res = pipe.recognize(frame, dets, top_k=3)
    assert [r["is_valid"] for r in res] == [i != 3 for i in range(8)]
    for i, r in enumerate(res):
        if i == 3:
            assert r["matches"] == []
            continue
        assert r["matches"][0][0] == f"S{i}" and abs(r["matches"][0][2] - 1.0) < 1e-5 and r["recognized"]
        assert r["quality_metrics"]["blur_score"] == A.blur_score(crops[i])
