"""The compact per-triangle record (semantic_meshes_amd/csrc/records.hpp), the part that needs no GPU: its pack / unpack helpers in a
stand-alone host program under AddressSanitizer / UBSan, and the option that selects the format."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_under_sanitizers(tmp_path):
    """tests/records_driver.cpp includes records.hpp and has its own main: round trips of random masks over every box size 1..8 x
    1..8 and the extreme origins, kind 3 exactly for small boxes over 6 pixels in x or y, the 36-bit order against the 64-bit
    order bit by bit, and the resolve's clear-bit index against the unpacked mask.  Run here, on the CPU."""
    exe = str(tmp_path / "records_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "records_driver.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "records driver ok" in out.stdout


def test_the_option_exists_and_round_trips():
    from semantic_meshes_amd import _lib
    before = _lib.get_option("compact_records")
    assert before in (0, 1)
    try:
        for v in (0, 1, 0):
            _lib.set_option("compact_records", v)
            assert _lib.get_option("compact_records") == v
    finally:
        _lib.set_option("compact_records", before)


def test_the_format_report_is_read_only_and_starts_at_16():
    """No raster launch can have happened in a process without a GPU; with one, the last launch left 8 or 16 bytes per record."""
    from semantic_meshes_amd import _lib
    assert _lib.get_option("last_record_format") in (8, 16)
    if _lib.device_count() == 0:
        assert _lib.get_option("last_record_format") == 16
    assert _lib.lib().smesh_set_option(b"last_record_format", 8) == _lib.ERR_INVALID
