"""Plain-text checks on the extension's source tree (no GPU, no build)."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "fmda_amd" / "ops" / "csrc"


def test_setup_lists_every_source_file():
    """setup.py compiles exactly the .hip / .cpp files under csrc/: a file
    left out of the list would silently drop its launchers from the .so.
    `*_hip.hip` are the build's own hipify copies (git-ignored)."""
    listed = set(re.findall(r'"fmda_amd/ops/csrc/([^"]+)"',
                            (ROOT / "setup.py").read_text()))
    present = {p.name for p in CSRC.iterdir()
               if p.suffix in (".hip", ".cpp")
               and not p.name.endswith("_hip.hip")}
    assert listed == present


def test_bindings_declares_no_launcher_itself():
    """Every launcher is declared once, in fmda_launch.h, which the
    defining files include too; an `extern "C"` redeclared by hand in
    bindings.cpp links even when its parameter list has drifted."""
    text = (CSRC / "bindings.cpp").read_text()
    assert 'extern "C"' not in text
    assert '#include "fmda_launch.h"' in text
