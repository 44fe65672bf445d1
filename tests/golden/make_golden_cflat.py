"""tests/golden/cflat.npz — fixtures of the experimental multi-vector weighted scan (experimental/multi_vector_vertex.go:85-137).

    python tests/golden/make_golden_cflat.py

Every answer comes from the INDEPENDENT pure-Python restatement (tests/cflat_ref.py) alone — never from the C++ oracle or the GPU, which
are the two things the file is there to pin (tests/test_cflat_ref.py: oracle == golden; tests/test_gpu_cflat.py: GPU == golden).  The
inputs are made here by integer arithmetic (splitmix64, a sum of four 16-bit uniforms: the same f32 bits on any machine) and are stored in
the file next to the answers, so a consumer needs neither this script nor a generator.  Rows of slot i are scaled by 1, 6 or 50
(i mod 3): the Euclidean score clamps at distance 100, and the store holds rows on both sides of it.  The archive is written with fixed
member timestamps, so a second run reproduces it byte for byte."""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
import cflat_ref as R  # noqa: E402

CFG = dict(n=300, nf=3, dim=12, nq=4, k=10, seed=9300)
RATIO_SETS = (([50, 30, 20], [1, 1, 1]), ([250, 0, 40], [1, 1, 0]))     # every field; a ratio above 100, a ratio 0 and an excluded field
SCALES = (1.0, 6.0, 50.0)


def _splitmix64(x):
    x = (x + np.uint64(0x9E3779B97F4A7C15))
    z = x
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def bell(seed, shape):
    """near-Gaussian f32 of about unit variance (the centred sum of four 16-bit uniforms): integers until ONE correctly rounded f32 division"""
    cnt = int(np.prod(shape))
    with np.errstate(over="ignore"):
        z = _splitmix64(np.arange(cnt, dtype=np.uint64) + np.uint64(seed * 0x100000001B3))
    s = np.zeros(cnt, np.int64)
    for j in range(4):
        s += ((z >> np.uint64(16 * j)) & np.uint64(0xFFFF)).astype(np.int64)
    return ((s - 2 * 65535).astype(np.float32) / np.float32(37837.0)).reshape(shape)   # sd of the sum = 65536 / sqrt(3)


def inputs():
    c = CFG
    X = bell(c["seed"], (c["n"], c["nf"], c["dim"]))
    X = X * np.array(SCALES, np.float32)[np.arange(c["n"]) % 3][:, None, None]
    Q = bell(c["seed"] + 1, (c["nq"], c["nf"], c["dim"]))
    ids = (np.arange(c["n"], dtype=np.uint64) * np.uint64(2654435761) + np.uint64(11)) % np.uint64(1 << 40)
    return X, Q, ids


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps (numpy stamps members with the wall clock)"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), version=(1, 0), allow_pickle=False)
            zi = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, buf.getvalue())


def arrays():
    c = CFG
    X, Q, ids = inputs()
    out = {"x_bits": X.view(np.uint32), "q_bits": Q.view(np.uint32), "ids": ids, "k": np.array([c["k"]], np.uint32),
           "ratios": np.array([r for r, _ in RATIO_SETS], np.uint32), "include": np.array([i for _, i in RATIO_SETS], np.uint8)}
    for metric in (R.COSINE, R.L2):
        ref = R.CFlatRef(c["dim"], c["nf"], metric)
        ref.upsert(ids, X)
        for si, (ratios, inc) in enumerate(RATIO_SETS):
            gi = np.zeros((c["nq"], c["k"]), np.uint64); gs = np.zeros((c["nq"], c["k"]), np.uint32)
            for qi in range(c["nq"]):
                i, s = ref.search(Q[qi], ratios, inc, c["k"])
                gi[qi] = i; gs[qi] = s.view(np.uint32)
            out[f"ids_{metric}_{si}"] = gi; out[f"scores_{metric}_{si}"] = gs
    return out


def main():
    out = arrays()
    save_npz(os.path.join(HERE, "cflat.npz"), out)
    print("wrote cflat.npz:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
