"""coltt_amd — MI355X-native ANN search hot path of sjy-dv/coltt.

The product is libcoltt_gpu.so (hand-written HIP for gfx950 behind the C-ABI of include/coltt_gpu.h).
This package is the thin ctypes binding used by tests/ and bench.py, shaped after the reference's Go
interfaces (edge.vectorspace: edge/vectorstore.go:30-49; *vectorindex.Hnsw: core/vectorindex/hnsw.go).
There is NO CPU fallback: importing works without a GPU (so the symbol table can be checked), but every
compute entry point fails loudly when the extension or the device is missing.
"""
from ._lib import (COSINE, EUCLIDEAN, Q_NONE, Q_F16, Q_F8, Q_BF16, SELECT_REFERENCE, SELECT_NEAREST,  # noqa: F401
                   MODE_EXACT, MODE_MFMA, ColttError, lib, lib_path, declared_symbols)
from .flat import FlatSpace  # noqa: F401
from .hnsw import Hnsw, HnswCfg, HnswFilter, FILTER_AUTO, FILTER_WALK, FILTER_EXACT  # noqa: F401
from .hnsw import HnswCompactStats, compact_map_host  # noqa: F401
from .hnsw import HnswCarryStats, carry_bits_host, carry_bits_device  # noqa: F401
from .hnsw import (PlanFactsC, SearchPlanC, search_plan_host, PLAN_LATENCY, PLAN_WALK2, PLAN_ONE_WAVE,  # noqa: F401
                   ROWF_UPPER_FILTER, ROWF_UPPER_CACHED)
from .hnsw import FOP_AND, FOP_OR, FOP_ANDNOT, FOP_NOT, FOP_ALL, filter_postfix, filter_tree, filter_prog_check  # noqa: F401
from .hnsw import (HnswAttrColumn, AttrPred, attr_cmp_host, ATTR_I64, ATTR_F64,  # noqa: F401
                   CMP_EQ, CMP_NE, CMP_GT, CMP_GE, CMP_LT, CMP_LE, CMP_SET)
from .cflat import MultiVectorSpace  # noqa: F401
from .pq import PQSpace, PQ_COSINE, PQ_EUCLIDEAN, PQ_DOT  # noqa: F401
from . import kernels  # noqa: F401
from . import group  # noqa: F401
from .group import Group  # noqa: F401
