"""training.ResidentTrainLoop under data parallelism (tests/rccl_loop_worker.py): a 1-rank RCCL group with GWTF_FORCE_SHARDED=1, the
only multi-rank configuration one GPU allows.  It has never run on more than one GPU.  Needs an MI355X."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_data_parallel_resident_loop_reduces_the_guard_flag_inside_the_graph():
    """The capture succeeds with the flag's MAX all-reduce inside; two replays give the plain resident loop's terms within 1e-5 (the
    bound of dist_model_worker.py); the trigger-NaN step skips the update.  The subprocess runs under `timeout`."""
    worker = os.path.join(os.path.dirname(__file__), 'rccl_loop_worker.py')
    r = subprocess.run(['timeout', '-k', '10', '240', sys.executable, worker], capture_output=True, text=True)
    assert r.returncode == 0 and 'LOOP1 ok' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
