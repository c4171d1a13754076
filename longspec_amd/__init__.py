"""longspec_amd -- MI355X-native draft-then-verify decode path of LongSpec.

Hand-written HIP kernels (gfx950) behind a C ABI (include/longspec_hip.h), driven
from PyTorch-ROCm through the reference's own Python API (`LlamaGlide`,
`tree_spec_generate`, ...).  See DESIGN.md.
"""
__version__ = "0.1.0"

from .sampling import Sampling  # noqa: E402,F401
from .penalties import Penalties  # noqa: E402,F401
from .logprobs import Logprobs  # noqa: E402,F401
from .stop import Stop  # noqa: E402,F401
from .ban import Ban  # noqa: E402,F401
from .guide import Guide  # noqa: E402,F401
from .dry import Dry  # noqa: E402,F401
from .watermark import Watermark  # noqa: E402,F401
from .cut import Cut  # noqa: E402,F401
from . import regex  # noqa: E402,F401
