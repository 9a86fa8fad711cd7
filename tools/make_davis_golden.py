"""Write tests/golden/davis_jf.npz: the results of the reference's OWN ``davis_db_eval_iou``, ``davis_db_eval_boundary`` and
``davis_db_statistics`` on the small seeded cases of tests/davis_reference.py.

    python tools/make_davis_golden.py --reference /path/to/NAF

Needs a checkout of the reference (valeoai/NAF) and scipy; ``evaluation/eval_video_seg.py`` is imported unmodified, on the CPU.  The
modules it imports at the top that the three functions do not need (hydra, omegaconf, torchvision, its own ``utils.training``, and rich /
tqdm / matplotlib / pandas / einops / PIL where they are missing) get empty stand-ins when they are not installed.  ``cv2`` is needed by
``_seg2bmap`` for ``cv2.filter2D``: when OpenCV is not installed the stand-in is ``scipy.ndimage.correlate(..., mode="mirror")`` -- a
correlation with the border reflected without repeating the edge, which is what OpenCV documents as its default (BORDER_REFLECT_101).  The
report in the fixture says which of the two was used.

The fixture holds, per case i of ``davis_reference.GOLDEN_CASES``: ``ann_i`` / ``seg_i`` uint8 [T, H, W], ``J_i`` / ``F_i`` fp64 [N, T],
``stats_J_i`` / ``stats_F_i`` fp64 [N, 3] (mean, recall, decay), ``bound_th_i``; and ``report``, a short text.
"""
import argparse
import importlib
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import davis_reference as R  # noqa: E402


def _stand_in(name, **attrs):
    try:
        importlib.import_module(name)
        return False
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
    return True


def _filter2d(src, ddepth, kernel):
    from scipy.ndimage import correlate
    return correlate(np.asarray(src), np.asarray(kernel), mode="mirror")


def import_reference(path):
    def main(*a, **k):
        return lambda f: f

    nothing = lambda *a, **k: None  # noqa: E731
    cv2_stood_in = _stand_in("cv2", filter2D=_filter2d)
    _stand_in("hydra", main=main)
    _stand_in("hydra.core")
    _stand_in("hydra.core.hydra_config", HydraConfig=object)
    _stand_in("hydra.utils", instantiate=nothing)
    _stand_in("omegaconf", DictConfig=dict, OmegaConf=object)
    _stand_in("rich", print=print)
    _stand_in("rich.console", Console=object)
    _stand_in("tqdm", tqdm=lambda it, **k: it)
    _stand_in("matplotlib")
    _stand_in("matplotlib.pyplot")
    _stand_in("pandas")
    _stand_in("einops", rearrange=nothing)
    _stand_in("PIL", Image=object)
    _stand_in("torchvision", transforms=object)
    sys.modules.pop("utils", None)          # the reference's own package: never the one of some other project
    sys.modules["utils"] = types.ModuleType("utils")
    sys.modules["utils"].__path__ = []
    sys.modules["utils.training"] = types.ModuleType("utils.training")
    sys.modules["utils.training"].load_multiple_backbones = nothing
    spec = importlib.util.spec_from_file_location("reference_eval_video_seg", os.path.join(path, "evaluation", "eval_video_seg.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, cv2_stood_in


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="checkout of the reference repository (the directory that holds evaluation/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "davis_jf.npz"))
    args = ap.parse_args()
    ref, cv2_stood_in = import_reference(args.reference)

    arrays = {}
    for ci in R.GOLDEN_CASES:
        H, W, T, N, bound_th, _ = R.CASES[ci]
        ann, seg = R.make_case(ci)
        J, F = np.zeros((N, T)), np.zeros((N, T))
        sJ, sF = np.zeros((N, 3)), np.zeros((N, 3))
        for o in range(1, N + 1):                         # the one-hot float arrays _evaluate_semisupervised hands over
            g, s = (ann == o).astype(np.float64), (seg == o).astype(np.float64)
            J[o - 1] = ref.davis_db_eval_iou(g, s, None)
            F[o - 1] = ref.davis_db_eval_boundary(g, s, None, bound_th=bound_th)
            sJ[o - 1] = ref.davis_db_statistics(J[o - 1])
            sF[o - 1] = ref.davis_db_statistics(F[o - 1])
        arrays.update({f"ann_{ci}": ann, f"seg_{ci}": seg, f"J_{ci}": J, f"F_{ci}": F, f"stats_J_{ci}": sJ, f"stats_F_{ci}": sF,
                       f"bound_th_{ci}": np.float64(bound_th)})
        print(f"case {ci} ({R.CASE_IDS[ci]}): mean J {J.mean():.6f}, mean F {F.mean():.6f}")
    report = ("davis_db_eval_iou, davis_db_eval_boundary (davis_f_measure, _seg2bmap) and davis_db_statistics are the reference's own code, "
              "imported unmodified from evaluation/eval_video_seg.py and run on the CPU with numpy %s and scipy's distance_transform_edt. " % np.__version__)
    if cv2_stood_in:
        report += ("OpenCV was NOT installed where this fixture was made: cv2.filter2D was stood in for by scipy.ndimage.correlate(mode='mirror'), "
                   "i.e. the border rule BORDER_REFLECT_101 is taken from OpenCV's documentation and is NOT pinned by this fixture; everything "
                   "else is the reference's code.")
    else:
        report += "cv2.filter2D was OpenCV's own (version %s): the border rule is pinned by this fixture." % sys.modules["cv2"].__version__
    arrays["report"] = np.array(report)
    np.savez_compressed(args.out, **arrays)
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes)\n{report}")


if __name__ == "__main__":
    main()
