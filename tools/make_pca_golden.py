"""Write tests/golden/P1_pca.npz: the results of the reference's OWN ``pca()`` (utils/visualization.py) on two square maps.

    python tools/make_pca_golden.py --reference /path/to/NAF

Needs a checkout of the reference (valeoai/NAF) and what its ``utils/visualization.py`` imports (matplotlib, einops, PIL); the file is
imported unmodified, on the CPU.  ``torch.pca_lowrank`` is randomised, so the reference runs under five ``torch.manual_seed`` values: the
fixture holds the first run and the largest deviation of the others from it.  Arrays only:

    maps             fp32 [2, 32, 12, 12]: tests/pca_reference.py golden_maps() (bf16 numbers)
    reduced_feats    fp32 [2, 3, 12, 12]: the reference's min-max normalised projections, seed 0
    components       fp32 [32, 3], mean fp32 [32], singular_values fp32 [3]: its TorchPCA, seed 0
    seeds            the seeds
    seed_spread      fp64: max over the other seeds and all elements of |reduced_feats - seed 0's|, each component compared up to the
                     flip y -> 1 - y (a component's sign is arbitrary)
"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pca_reference as R  # noqa: E402

SEEDS = (0, 1, 2, 3, 4)


def import_reference(path):
    import matplotlib
    matplotlib.use("Agg")
    spec = importlib.util.spec_from_file_location("reference_visualization", os.path.join(path, "utils", "visualization.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="checkout of the reference repository (the directory that holds utils/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "P1_pca.npz"))
    args = ap.parse_args()
    ref = import_reference(args.reference)

    maps = R.golden_maps()
    runs = []
    for seed in SEEDS:
        torch.manual_seed(seed)
        reduced, fit = ref.pca([m.clone() for m in maps], dim=3)
        runs.append((torch.cat([r.float() for r in reduced], dim=0), fit))
    first, fit0 = runs[0]
    spread = max(R.match_up_to_flip(run[i:i + 1], first[i:i + 1]) for run, _ in runs[1:] for i in range(len(maps)))
    np.savez(args.out, maps=torch.cat(maps, dim=0).numpy(), reduced_feats=first.numpy(), components=fit0.components_.float().numpy(),
             mean=fit0.mean_.float().numpy(), singular_values=fit0.singular_values_.float().numpy(), seeds=np.array(SEEDS),
             seed_spread=np.float64(spread))
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes): seed spread {spread:.3e}, singular values {fit0.singular_values_.tolist()}")


if __name__ == "__main__":
    main()
