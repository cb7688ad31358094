import glob
import os
import re
import sys

# ROCm 7.2: with the runtime's AQL-packet capture on (the default) a MEMSET node of a replayed hipGraph is not ordered
# behind the kernels before it (tools/graph_memset_probe.py); torch's multi-block reductions, and whatever else a
# library zeroes that way, then read garbage from the second replay on.  Read when the HIP runtime loads.
os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def pytest_collection_modifyitems(config, items):
    """``gpu``-marked tests need a device: skip them (instead of erroring) on a host without one."""
    import torch
    if torch.cuda.is_available():
        return
    skip = pytest.mark.skip(reason="needs a GPU (MI355X): run with -m gpu on the GPU box")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip)


# A fixture is <name>.npz plus, when its arrays do not fit one file of GOLDEN_PART_BYTES, <name>.1.npz, <name>.2.npz, ...
GOLDEN_PART_BYTES = 960_000
_PART = re.compile(r"\.[0-9]+\.npz$")


def golden_cases(pattern="msda_*.npz"):
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, pattern)) if not _PART.search(p))


def load_npz(path):
    """Every array of the fixture ``path`` (<name>.npz) and of its parts <name>.<i>.npz."""
    stem = path[:-4]
    parts = sorted(glob.glob(glob.escape(stem) + ".[0-9]*.npz"), key=lambda p: int(p[len(stem) + 1:-4]))
    arrays = {}
    for p in [path] + [p for p in parts if _PART.search(p)]:
        with np.load(p) as z:
            arrays.update({k: z[k] for k in z.files})
    return arrays


def save_npz(path, **arrays):
    """np.savez_compressed of ``arrays`` as <name>.npz and, past GOLDEN_PART_BYTES, parts <name>.1.npz, ... (arrays
    whole, in order; one array per file at most when it is larger on its own).  load_npz reads them back."""
    import io
    stem = path[:-4]
    for p in glob.glob(glob.escape(stem) + ".[0-9]*.npz"):
        if _PART.search(p):
            os.remove(p)

    def packed(group):
        buf = io.BytesIO()
        np.savez_compressed(buf, **group)
        return buf.getvalue()

    files, group, data = [], {}, packed({})
    for k, v in arrays.items():
        trial = packed(dict(group, **{k: v}))
        if group and len(trial) > GOLDEN_PART_BYTES:
            files.append(data)
            group, trial = {}, packed({k: v})
        group[k], data = v, trial
    files.append(data)
    for i, data in enumerate(files):
        with open(path if i == 0 else f"{stem}.{i}.npz", "wb") as f:
            f.write(data)


def load_golden(name):
    return load_npz(os.path.join(GOLDEN_DIR, name + ".npz"))


@pytest.fixture(scope="session")
def hip_lib():
    """The product library; built on demand (hipcc cross-compiles without a GPU)."""
    from memotr_amd.build import build_lib
    build_lib()
    from memotr_amd import _lib
    return _lib


@pytest.fixture(scope="session")
def clip_lib():
    """libclip_ops_hip.so (fused small-tensor chains of the train step); built on demand."""
    from memotr_amd.build import build_clip_lib
    build_clip_lib()
    from memotr_amd import _clip_lib
    return _clip_lib


def has_gpu():
    import torch
    return torch.cuda.is_available()


_TEST_SITE = [1 << 40]


@pytest.fixture(autouse=True)
def _fresh_call_site(request):
    """Kernel selection keeps one record per CALL SITE (memotr_amd/csrc/msda_select.h; round 5: no longer per geometry --
    the measured off-window share is a property of a module's learnt offsets).  Direct operator calls of a test are
    untagged, so without this every GPU test would inherit the level the previous test's data left behind: each GPU
    test gets a call site of its own (the model's modules tag their calls themselves)."""
    if "gpu" not in request.keywords or not has_gpu():
        yield
        return
    from memotr_amd import MultiScaleDeformableAttention as MSDA
    from memotr_amd import _lib
    # ... and starts without records: msda_selector_poll()'s signature covers every record of the device, those of
    # earlier tests' modules included (a record left at the top level announces a probe every 32nd poll, and a graph
    # cache of the next test captures once more than that test counts on)
    _lib.selector_reset()
    _TEST_SITE[0] += 1
    MSDA.set_call_site(_TEST_SITE[0])
    yield
    MSDA.set_call_site(0)
