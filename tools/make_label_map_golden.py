"""Write tests/golden/pil_nearest_tables.npz: the source indices Pillow's ``Image.resize(size, 0)`` (nearest) reads, recorded from Pillow
itself, for the (n_in, n_out) pairs of ``label_map_reference.FIXTURE_PAIRS`` -- the DAVIS sizes and every pair the label-map tests resize
with.  The GPU tests compare the library's tables against this fixture where Pillow is not installed.

    python tools/make_label_map_golden.py

Needs Pillow.  Every pair is read along both axes of an ``I`` (int32) image whose pixels hold their own index, and along both axes of an
``L`` image as well where the indices fit a byte; the four readings must agree.  The fixture holds ``pairs`` int32 [n, 2], one int32 array
``t_<n_in>_<n_out>`` per pair, and ``pillow``, the version that made it.
"""
import os
import sys

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import label_map_reference as R  # noqa: E402


def pillow_table(n_in, n_out):
    readings = []
    for dtype in ([np.int32, np.uint8] if n_in <= 256 else [np.int32]):
        idx = np.arange(n_in, dtype=dtype)
        along_x = np.array(Image.fromarray(np.repeat(idx[None], 3, 0)).resize((n_out, 3), 0))
        along_y = np.array(Image.fromarray(np.repeat(idx[:, None], 3, 1)).resize((3, n_out), 0))
        assert (along_x == along_x[:1]).all() and (along_y == along_y[:, :1]).all()
        readings += [along_x[0].astype(np.int32), along_y[:, 0].astype(np.int32)]
    for r in readings[1:]:
        assert np.array_equal(r, readings[0]), (n_in, n_out)
    return readings[0]


def main():
    arrays = {"pairs": np.array(R.FIXTURE_PAIRS, dtype=np.int32), "pillow": np.array(PIL.__version__)}
    for n_in, n_out in R.FIXTURE_PAIRS:
        arrays[f"t_{n_in}_{n_out}"] = pillow_table(n_in, n_out)
    path = os.path.join(ROOT, "tests", "golden", "pil_nearest_tables.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {len(R.FIXTURE_PAIRS)} pairs from Pillow {PIL.__version__}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
