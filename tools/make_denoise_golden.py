"""Write tests/golden/denoise_objective.npz: the results of the reference's OWN ``DenoisingLoss`` and ``MetricsCalculator`` on one input pair.

    python tools/make_denoise_golden.py --reference /path/to/NAF

Needs a checkout of the reference (valeoai/NAF); its ``denoising.py`` is imported unmodified, on the CPU.  The modules it imports at
the top that are not needed for the two classes (hydra, omegaconf, rich, tqdm, its own ``utils.training``) get empty stand-ins when they
are not installed.  The fixture holds arrays only:

    pred, target                     fp32 [2, 3, 20, 24] (tests/denoise_reference.py: make_inputs, unclamped variant)
    l1, l2, ssim, total, grad        DenoisingLoss(1.0, 5.0, 0.2) in fp64 on the widened inputs, grad = d total / d pred by total.backward()
    psnr, ssim_metric                MetricsCalculator.calculate_batch_metrics in fp32 on torch.clamp(pred, 0, 1)
"""
import argparse
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import denoise_reference as R  # noqa: E402


def _stand_in(name, **attrs):
    try:
        importlib.import_module(name)
        return
    except Exception:
        pass
    mod = types.ModuleType(name)
    mod.__path__ = []
    for k, v in attrs.items():
        setattr(mod, k, v)
    sys.modules[name] = mod
    if "." in name:
        parent, child = name.rsplit(".", 1)
        setattr(sys.modules[parent], child, mod)


def import_reference(path):
    def main(*a, **k):
        return lambda f: f

    nothing = lambda *a, **k: None  # noqa: E731
    _stand_in("hydra", main=main)
    _stand_in("hydra.core")
    _stand_in("hydra.core.hydra_config", HydraConfig=object)
    _stand_in("hydra.utils", instantiate=nothing)
    _stand_in("omegaconf", DictConfig=dict, OmegaConf=object)
    _stand_in("rich", print=print)
    _stand_in("rich.console", Console=object)
    _stand_in("rich.syntax", Syntax=object)
    _stand_in("tqdm", tqdm=lambda it, **k: it)
    sys.modules.pop("utils", None)          # the reference's own package: never the one of some other project
    sys.modules["utils"] = types.ModuleType("utils")
    sys.modules["utils"].__path__ = []
    sys.modules["utils.training"] = types.ModuleType("utils.training")
    for name in ("get_batch", "get_dataloaders", "logger", "setup_training_optimizations"):
        setattr(sys.modules["utils.training"], name, nothing)
    spec = importlib.util.spec_from_file_location("reference_denoising", os.path.join(path, "denoising.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="checkout of the reference repository (the directory that holds denoising.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "denoise_objective.npz"))
    args = ap.parse_args()
    ref = import_reference(args.reference)

    pred, target = R.make_inputs(R.GOLDEN_SHAPE, clamped=False)
    p64 = pred.double().requires_grad_(True)
    losses = ref.DenoisingLoss(*R.GOLDEN_WEIGHTS)(p64, target.double())
    losses["total"].backward()
    m = ref.MetricsCalculator.calculate_batch_metrics(torch.clamp(pred, 0, 1), target)
    np.savez(args.out, pred=pred.numpy(), target=target.numpy(),
             l1=np.float64(losses["l1"].item()), l2=np.float64(losses["l2"].item()), ssim=np.float64(losses["ssim"].item()),
             total=np.float64(losses["total"].item()), grad=p64.grad.numpy(),
             psnr=np.float64(m["psnr"]), ssim_metric=np.float64(m["ssim"]))
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes): total {losses['total'].item():.12g}, psnr {m['psnr']:.6f} dB, ssim {m['ssim']:.8f}")


if __name__ == "__main__":
    main()
