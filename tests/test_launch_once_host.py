"""CPU: the dynamic-LDS limit of a kernel is raised in one place, hsp::launch_lds (csrc/common.h), on every launch above 64 KiB
-- the attribute is a per-device setting, so no source may raise it by hand or remember in a per-process flag that it did.
Reads the sources as text; needs no library."""
import pathlib

CSRC = pathlib.Path(__file__).resolve().parent.parent / "hs_pose_amd" / "csrc"


def _sources():
    files = sorted(p for p in CSRC.iterdir() if p.suffix in (".hip", ".h", ".cpp"))
    assert len(files) > 20 and CSRC / "common.h" in files
    return {p.name: p.read_text() for p in files}


def test_limit_raised_in_common_h_only():
    users = [name for name, text in _sources().items() if "hipFuncSetAttribute" in text]
    assert users == ["common.h"], f"hipFuncSetAttribute outside launch_lds: {users}"


def test_no_per_process_flag():
    users = [name for name, text in _sources().items() if "attr_set" in text]
    assert users == [], f"a per-process 'limit already raised' flag: {users}"
