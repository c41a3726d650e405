"""Run bench.py with the per-point chains on their software-pipelined entry points (fused.PW_ENTRIES_PIPELINED): the third arm of a
same-box comparison, which separates the pipelined tile loops from anything else in the build.
    python tools/experiments/bench_pw_pipelined.py [bench.py arguments]"""
import os, runpy, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from ratrack_amd import fused as F
F.PW_ENTRIES = F.PW_ENTRIES_PIPELINED
sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[1:]
runpy.run_path(os.path.join(ROOT, "bench.py"), run_name="__main__")
