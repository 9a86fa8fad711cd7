"""The boundary of ``naf_amd.ops`` (CPU, no library load): every name the rest of the tree reaches through it resolves on it, and the
kernel timer is ONE global there that ``_Timed`` reads at call time.  Both must keep holding however the operators are laid out in files."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
USE = re.compile(r"(?<![\w.])ops\.([A-Za-z_]\w*)")
# what the scan finds on the tree this test was added to: 138 sources, 99 distinct names.  Fewer means the scan lost its sources.
MIN_FILES, MIN_NAMES = 138, 99


def test_ops_surface_and_single_kernel_timer():
    import naf_amd.ops
    from naf_amd import ops
    assert ops is naf_amd.ops
    # (a) every attribute of ``ops`` written anywhere outside its own sources resolves on it
    own = os.path.join(ROOT, "naf_amd", "ops")
    own = (own + os.extsep + "py", own + os.sep)          # the module today, or a package of that name
    files = [f for pat in ("naf_amd/*.py", "tools/*.py", "tests/*.py", "*.py", "examples/**/*.py")
             for f in glob.glob(os.path.join(ROOT, pat), recursive=True) if not f.startswith(own)]
    used = {}
    for f in files:
        with open(f, encoding="utf-8") as fh:
            for name in USE.findall(fh.read()):
                used.setdefault(name, os.path.relpath(f, ROOT))
    missing = {n: f for n, f in used.items() if not hasattr(ops, n)}
    assert not missing, f"used through naf_amd.ops but not defined there: {missing}"
    assert len(files) >= MIN_FILES and len(used) >= MIN_NAMES, (len(files), len(used))

    # (b) a timer assigned on ``ops`` is what _Timed sees, from wherever a launch wrapper reaches _Timed
    assert ops.KERNEL_TIMER is None

    class Recorder:
        def __init__(self):
            self.seen = []

        def start(self, name):
            self.seen.append(("start", name))

        def stop(self, name):
            self.seen.append(("stop", name))

    wrappers = (ops.stem_conv0, ops.xna_forward, ops.xna_head_forward, ops.propagate_labels, ops.prepare_views, ops.denoise_objective,
                ops.feature_moments)                                   # one launch wrapper of every family that times its launches
    ops.KERNEL_TIMER = rec = Recorder()
    try:
        for fn in wrappers:
            with fn.__globals__["_Timed"]("x"):
                pass
            assert rec.seen == [("start", "x"), ("stop", "x")], (fn.__name__, rec.seen)
            rec.seen.clear()
    finally:
        ops.KERNEL_TIMER = None
    with ops._Timed("x"):      # no timer: nothing is called
        pass
    assert rec.seen == []
