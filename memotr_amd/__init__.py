"""memotr_amd -- MI355X-native (gfx950) hot path of MeMOTR.

Package layout mirrors the reference's interface for the path it replaces:

  memotr_amd.csrc/                      hand-written HIP kernels + the C ABI (include/msda_hip.h)
  memotr_amd.MultiScaleDeformableAttention   same two entry points as the reference's compiled
                                        extension (models/ops/src/vision.cpp:13-16)
  memotr_amd.functions / .modules       MSDeformAttnFunction / MSDeformAttn
                                        (models/ops/functions, models/ops/modules)
  memotr_amd.models / .structures / .utils   per-frame model path (models/memotr.py etc.)

The HIP library is mandatory: importing the operator without a built
``memotr_amd/lib/libmsda_hip.so`` raises (there is no CPU fallback in the product).
"""

import os as _os

# hipGraph replays on ROCm 7.2 mis-order memset nodes unless the runtime's AQL-packet capture is off (see
# models/graph_capture.py, tools/graph_memset_probe.py).  The runtime reads the flag when it loads, i.e. this only
# helps when the package is imported before torch; bench.py / the tests / __graft_entry__ set it themselves.  The
# captured regions of this package contain no memset nodes either way (held by the GPU tests).
_os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")

__version__ = "0.1.0"
