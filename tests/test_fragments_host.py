"""The packed fragment-queue entry (semantic_meshes_amd/csrc/fragments.hpp), the part that needs no GPU: its pack / unpack helpers in a
stand-alone host program under AddressSanitizer / UBSan, and the option that selects the format."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_under_sanitizers(tmp_path):
    """tests/fragments_driver.cpp includes fragments.hpp and has its own main: round trips at the extremes of every field (id 0 and
    2^22 - 1, pixel 0 and 2047, z bits 1, FLT_MIN, FLT_MAX), the packed order against the key order for random pairs at one pixel
    (equal z included), null above background above every fragment, and the predicate (F = 2^22 yes, 2^22 + 1 no, texels no).
    Run here, on the CPU."""
    exe = str(tmp_path / "fragments_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "fragments_driver.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "fragments driver ok" in out.stdout


def test_the_option_exists_and_round_trips():
    from semantic_meshes_amd import _lib
    before = _lib.get_option("packed_fragments")
    assert before in (0, 1)
    try:
        for v in (0, 1, 0):
            _lib.set_option("packed_fragments", v)
            assert _lib.get_option("packed_fragments") == v
    finally:
        _lib.set_option("packed_fragments", before)


def test_the_format_report_is_read_only_and_starts_at_10():
    """No raster launch can have happened in a process without a GPU; with one, the last launch queued 8 or 10 bytes per fragment."""
    from semantic_meshes_amd import _lib
    assert _lib.get_option("last_fragment_format") in (8, 10)
    if _lib.device_count() == 0:
        assert _lib.get_option("last_fragment_format") == 10
    assert _lib.lib().smesh_set_option(b"last_fragment_format", 8) == _lib.ERR_INVALID
