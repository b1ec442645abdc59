"""Raw bytes of the last-layer class's results below 129 units, for a library-against-library comparison (profiles/wide_ll_ab.md):
every ll_* case of tests/test_gpu_parity.CONFIGS -- forward and [grad | loss] of the plain and of the sample-weighted step -- written to
one file per case under --out.  Run once per library (NIF_LIB selects it), then compare the directories:

    NIF_LIB=/path/to/parent/libnif_hip.so python tools/ab_ll_bytes.py --out ab_out/parent
    python tools/ab_ll_bytes.py --out ab_out/this
    python tools/ab_ll_bytes.py --compare ab_out/parent ab_out/this"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def write(out):
    from tests.test_gpu_parity import CONFIGS, _make
    os.makedirs(out, exist_ok=True)
    for name in sorted(k for k in CONFIGS if k.startswith("ll_")):
        m, model, spec, ws, x, y, sw = _make(name)
        parts = [model.predict(x).tobytes()]
        for s in (None, sw):
            loss, g = m._engine.loss_and_grad(x, y, s)
            parts += [g.tobytes(), np.float32(loss).tobytes()]
        with open(os.path.join(out, name + ".bin"), "wb") as f:
            f.write(b"".join(parts))
        print(name, sum(len(p) for p in parts), "bytes")


def compare(a, b):
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and names, (names, sorted(os.listdir(b)))
    bad = 0
    for nm in names:
        da, db = open(os.path.join(a, nm), "rb").read(), open(os.path.join(b, nm), "rb").read()
        same = da == db
        bad += not same
        print("%-28s %9d bytes  %s" % (nm, len(da), "identical" if same else "DIFFERENT"))
    print("%d cases, %d identical, %d different" % (len(names), len(names) - bad, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", nargs=2, default=None)
    args = ap.parse_args()
    sys.exit(compare(*args.compare) if args.compare else write(args.out))
