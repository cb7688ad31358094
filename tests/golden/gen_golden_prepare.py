"""Golden files for dataset preparation (memotr_amd/data/prepare.py), produced by the REFERENCE's own
``data/gen_mot17_gts.py``, ``data/gen_crowdhuman_gts.py`` and ``data/gen_bdd100k_gts.py`` on the input trees of
tests/prepare_trees.py (needs a checkout of the reference; the tests that read the fixture do not):

    python tests/golden/gen_golden_prepare.py --reference /path/to/reference   ->  tests/golden/prepare.json

The three scripts are read from that checkout and executed as they are, as ``__main__``, with two things arranged in
memory: every string literal that names the author's dataset directory is replaced by the same path under a temporary
DATA_ROOT, and ``cv2`` (``imread`` gives a blank image: the scripts use its shape for nothing) and ``tqdm`` are stood in
for in ``sys.modules``.  ``os.listdir`` returns sorted names while they run, which is the order prepare.py takes.  The
BDD100K script calls its ``generate_txt`` in comments only; it is called here from the executed namespace, on the
filtered labels.

Recorded: {"mot17" | "crowdhuman" | "bdd100k": {path relative to DATA_ROOT: text}} of every file the scripts wrote.
"""
import argparse
import contextlib
import io
import json
import os
import re
import sys
import tempfile
import types

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))              # tests/: prepare_trees

MARK = "DatasetsForMeMOTR"                            # the directory name the scripts' path literals share


def install_stand_ins():
    import numpy as np
    cv2 = types.ModuleType("cv2")
    cv2.IMREAD_COLOR, cv2.IMREAD_IGNORE_ORIENTATION = 1, 128
    cv2.imread = lambda path, flags=None: np.zeros((8, 8, 3), dtype=np.uint8)
    tqdm = types.ModuleType("tqdm")
    tqdm.tqdm = lambda iterable, *a, **k: iterable
    sys.modules["cv2"], sys.modules["tqdm"] = cv2, tqdm


def run_script(path, root):
    """Execute the script at ``path`` as ``__main__`` with its dataset literals under ``root``; returns its namespace."""
    with open(path) as f:
        source = f.read()
    pattern = re.compile(r"""(["'])[^"'\n]*""" + MARK + r"""([^"'\n]*)\1""")
    source, n = pattern.subn(lambda m: repr(root + m.group(2)), source)
    assert n > 0, f"{path}: no path literal found"
    namespace = {"__name__": "__main__", "__file__": path}
    with contextlib.redirect_stdout(io.StringIO()):
        exec(compile(source, path, "exec"), namespace)
    return namespace


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference (its data/gen_*_gts.py are run)")
    args = ap.parse_args()
    import prepare_trees as trees
    data = os.path.join(os.path.abspath(args.reference), "data")
    if not os.path.exists(os.path.join(data, "gen_mot17_gts.py")):
        raise SystemExit(f"{data}/gen_mot17_gts.py does not exist: --reference must name a checkout")
    install_stand_ins()
    listdir = os.listdir
    os.listdir = lambda *a, **k: sorted(listdir(*a, **k))
    try:
        with tempfile.TemporaryDirectory(prefix="prepare_") as root:
            trees.write_inputs(root)
            run_script(os.path.join(data, "gen_mot17_gts.py"), root)
            run_script(os.path.join(data, "gen_crowdhuman_gts.py"), root)
            bdd = run_script(os.path.join(data, "gen_bdd100k_gts.py"), root)
            bdd["generate_txt"](os.path.join(root, "BDD100K", "images", "track"),
                                os.path.join(root, "BDD100K", "filter_labels", "track"),
                                txt_path=os.path.join(root, "BDD100K", "filter.bdd100k.train"), split="train")
            recorded = trees.read_outputs(root)
    finally:
        os.listdir = listdir
    path = os.path.join(OUT, "prepare.json")
    with open(path, "w") as f:
        json.dump(recorded, f, indent=1, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes,", {k: len(v) for k, v in recorded.items()}, "files")


if __name__ == "__main__":
    main()
