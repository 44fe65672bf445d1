import numpy as np


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def assert_same_results(got_ids, got_sc, want_ids, want_sc, msg=""):
    assert len(got_ids) == len(want_ids), f"{msg}: count {len(got_ids)} != {len(want_ids)}"
    assert np.array_equal(np.asarray(got_ids, np.uint64), np.asarray(want_ids, np.uint64)), f"{msg}: ids differ\n{got_ids}\n{want_ids}"
    assert np.array_equal(bits(got_sc), bits(want_sc)), f"{msg}: score bits differ\n{got_sc}\n{want_sc}"


# ---- shared by the multi-vector scan's CPU and GPU tests (test_cflat_ref.py, test_gpu_cflat.py)
def cflat_ratio_sets(nf):
    """(ratios, include) per field: every field included ([50, 30, 20] at nf = 3); ratio 0 on an included field; a ratio of 250;
    every field excluded; one included field only"""
    base = [50, 30, 20, 45, 5, 60, 10, 80][:nf]
    ones = [1] * nf
    zero = list(base); zero[nf - 1] = 0
    big = list(base); big[0] = 250
    one = [0] * nf; one[nf // 2] = 1
    return [(base, ones), (zero, ones), (big, ones), (base, [0] * nf), (base, one)]


def cflat_scaled_rows(X):
    """rows of slot i times 1, 6 or 50 (i mod 3): against a Gaussian query the Euclidean distances lie well below 100, around it and far
    above it, so scoreHelper's clamp max(0, 100 - d) fires for some rows and not for others"""
    s = np.array([1, 6, 50], np.float32)[np.arange(len(X)) % 3]
    return (X * s.reshape((-1,) + (1,) * (X.ndim - 1))).astype(np.float32)
