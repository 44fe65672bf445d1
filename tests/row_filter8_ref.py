"""The ingest quantiser of the 8-bit row-filter shadow (coltt_amd/csrc/rows8_ingest.hpp: rows_b_kernel), restated in numpy for the tests that check the
bound (test_row_filter8_bound.py) and the device's arrays (test_gpu_row_filter8.py)."""
import math

import numpy as np


def quantise(x):
    """rows8_ingest.hpp: rows_b_kernel — (s, codes, stored e) of one f32 row; a zero row, a row with a non-finite element and a scale that underflows
    to 0 get codes 0, s = 0 and e = +inf"""
    x = np.ascontiguousarray(x, np.float32)
    none = (np.zeros(x.size, np.int8), np.float32(0), np.float32(np.inf))
    if not np.all(np.isfinite(x)):
        return none
    s = np.float32(np.max(np.abs(x)) / np.float32(127))      # one f32 division
    if not s > 0:
        return none
    with np.errstate(over="ignore"):
        c = np.clip(np.rint((x / s).astype(np.float32)), -127, 127)   # f32 division, ties to even
    d = x.astype(np.float64) - np.float64(s) * c.astype(np.float64)   # the product is exact in f64
    ev = math.sqrt(float(np.sum(d * d))) * (1.0 + 2.0 ** -20)
    e = np.float32(ev)
    if float(e) < ev:
        e = np.nextafter(e, np.float32(np.inf), dtype=np.float32)     # towards +infinity
    return c.astype(np.int8), s, e
