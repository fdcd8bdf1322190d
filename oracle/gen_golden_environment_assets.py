"""tests/golden/environment_assets.npz: the reference's obstacle URDFs the asset tests read, packed as text (one string array
per file, key "<set>__<file>"): every file of objects / panels / walls and the first 25 (by number) of trees / thin.

    python oracle/gen_golden_environment_assets.py        (in the build container: needs the reference tree)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from ref_shells import REFERENCE_ROOT  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden", "environment_assets.npz")


def main():
    src = os.path.join(REFERENCE_ROOT, "resources", "models", "environment_assets")
    files = {sub: sorted(f for f in os.listdir(os.path.join(src, sub)) if f.endswith(".urdf")) for sub in ("objects", "panels", "walls")}
    files.update({sub: [f"{stem}_{i}.urdf" for i in range(25)] for sub, stem in (("trees", "tree"), ("thin", "thin"))})
    out = {f"{sub}__{f}": np.array(open(os.path.join(src, sub, f)).read()) for sub, names in files.items() for f in names}
    np.savez_compressed(OUT, **out)
    print(OUT, len(out), "files")


if __name__ == "__main__":
    main()
