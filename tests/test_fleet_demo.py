"""The fleet demo (examples/fleet_demo.py) runs clean on CPU."""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fleet_demo():
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "examples", "fleet_demo.py"),
         "--hidden", "16", "--symbols", "3", "--window", "8", "--ticks", "2"],
        capture_output=True, text=True, timeout=120, cwd=REPO)
    assert out.returncode == 0, out.stderr[-800:]
    assert "6 predictions published in 2 fleet ticks" in out.stdout
