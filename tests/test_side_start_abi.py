"""StTuning::side_start on a host-only engine: the default is one of the documented values, set / get round-trips, a value past 3 is
refused, and ST_SIDE_START overrides the default when an engine is created. (What the value does: tests/test_gpu_side_schedule.py.)"""
import os
import subprocess
import sys

import pytest

from strolle_amd import Engine
from strolle_amd.api import StrolleError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_side_start_round_trips_and_is_validated():
    e = Engine(device=-1)
    assert e.tuning().side_start in range(4)
    for v in range(4):
        e.set_tuning(side_start=v)
        assert e.tuning().side_start == v
    with pytest.raises(StrolleError):
        e.set_tuning(side_start=4)
    assert e.tuning().side_start == 3, "a refused StTuning changes nothing"
    e.close()


def test_the_environment_overrides_the_default():
    code = "from strolle_amd import Engine; e = Engine(device=-1); print(e.tuning().side_start); e.close()"
    for v in ("0", "2"):
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, ST_SIDE_START=v), capture_output=True, text=True, check=True)
        assert out.stdout.split()[-1] == v
