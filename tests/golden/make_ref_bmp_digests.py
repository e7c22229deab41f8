"""Generates tests/golden/ref_bmp_digests.json: the bytes the reference's own stbi_write_bmp writes for the inputs of the BMP tests.

The reference's BMP writer is its vendored stb_image_write.h, compiled by `make -C oracle` into oracle/_ref/libref_bmp.so only where
the reference tree is present. The tests compare the oracle's and the library's BMP writers against these recorded SHA-256 digests,
so that they hold on every machine, and against the compiled writer itself as well where it was built.
Run where oracle/_ref/libref_bmp.so exists:   python tests/golden/make_ref_bmp_digests.py
"""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from golden_util import REF_BMP_DIGESTS, ref_bmp_key   # noqa: E402
from oracle import binding as ob                      # noqa: E402


def inputs():
    """Every image the BMP tests hand to a writer, generated as the tests generate them."""
    rng = np.random.default_rng
    # tests/test_oracle_kat.py::test_bmp_matches_reference_stb
    for w, h in [(3, 3), (4, 2), (5, 7), (492, 492), (1, 1)]:
        yield rng(w * 100 + h).integers(0, 256, size=(h, w), dtype=np.uint8)
    # tests/test_oracle_kat.py::test_rgba_bmp_matches_reference_stb
    yield rng(77).integers(0, 256, size=(5, 7, 4), dtype=np.uint8)
    for w, h in [(1, 1), (512, 128), (3, 2)]:
        yield rng(w + h).integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    # tests/test_abi.py::test_host_io_matches_oracle_and_reference_stb
    r = rng(5)
    for w, h in [(3, 3), (5, 2), (492, 492)]:
        yield r.integers(0, 256, size=(h, w), dtype=np.uint8)
    for w, h in [(512, 128), (3, 2), (1, 1)]:
        yield r.integers(0, 256, size=(h, w, 4), dtype=np.uint8)


def main():
    ob.build()
    if not ob.ref_bmp_available():
        raise SystemExit("oracle/_ref/libref_bmp.so is not built (the reference tree was absent when the oracle was built)")
    res = {}
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "ref.bmp")
        for data in inputs():
            (ob.ref_write_bmp_rgba if data.ndim == 3 else ob.ref_write_bmp_gray)(path, data)
            with open(path, "rb") as f:
                res[ref_bmp_key(data)] = hashlib.sha256(f.read()).hexdigest()
    with open(REF_BMP_DIGESTS, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d digests -> %s" % (len(res), REF_BMP_DIGESTS))


if __name__ == "__main__":
    main()
