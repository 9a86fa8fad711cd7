"""naf_amd/csrc/stem_rows_sched.inc is committed, and the build does not run its generator: the file must be exactly what
tools/gen_stem_rows.py emits."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_committed_schedule_is_the_generators_output(tmp_path):
    out = tmp_path / "sched.inc"
    env = {k: v for k, v in os.environ.items() if not k.startswith("NAF_ROWS_")}      # the generator's tuning knobs
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_stem_rows.py"), str(out)], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(os.path.join(ROOT, "naf_amd", "csrc", "stem_rows_sched.inc"), "rb") as fh:
        committed = fh.read()
    assert out.read_bytes() == committed
