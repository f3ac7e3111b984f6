"""pgrc_amd -- MI355X-native implementation of PgRC's read-to-pseudogenome matching path.

The product is `libpgrc_match.so` (hand-written HIP kernels for gfx950 behind the C ABI of
`include/pgrc_match.h`).  This package is the thin host-side mirror of the reference's matcher
interface (matching/ReadsMatchers.h) on top of that ABI; it contains no compute of its own.
"""
from ._lib import LIB_PATH, NOT_MATCHED_CNT, NOT_MATCHED_POS, PgrcMatchError  # noqa: F401
from .matchers import (  # noqa: F401
    AbstractReadsApproxMatcher,
    CopMEMReadsApproxMatcher,
    DefaultReadsApproxMatcher,
    DefaultReadsExactMatcher,
    DefaultReadsMatcher,
    InterleavedReadsApproxMatcher,
    MatchContext,
    copmem_params,
    mapReadsIntoPg,
)
from .textmatch import CopMEMMatcher  # noqa: F401
from .readsets import DividedPCLReadsSets, DividedReadsSets, reads_text_format  # noqa: F401
from . import synth  # noqa: F401
from .decode import (  # noqa: F401
    PgRCDecoder,
    compressReadsOrder,
    compressReadsPgPositions,
    decompressReadsOrder,
    decompressReadsPgPositions,
)
from .assemble import PgAssembler  # noqa: F401
from .overlap import OverlapFinder  # noqa: F401
from .varlen import VarLenDNACoder  # noqa: F401
from .huf import HufCoder  # noqa: F401
from .rlist import ReadsList  # noqa: F401
from .verify import Verifier  # noqa: F401
from . import archive  # noqa: F401
from .pipeline import compress, decompress  # noqa: F401
