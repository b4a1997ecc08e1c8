"""csrc/bds_record_window.h, the window of a record file that bds_blank_file, bds_notch_file and bds_probe_data_file share, in a
stand-alone program under AddressSanitizer and UBSan (tests/host_models/record_window_check.cpp), with no GPU and no library.
Every expected value is computed here from the definitions: the file's size, the format's bits per sample, the skip."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = {0: 8, 1: 16, 2: 4, 3: 16, 4: 32}  # probe::Format: s8, s8c, packed 2+2-bit I/Q, s16, s16c
PACKED = 2
ERR_ARG, ERR_IO = -1, -4
SIZE = 101  # bytes: odd, so that the last sample of every wider format is cut


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("window") / "record_window_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "bds-3-b1c-b2a-sdr-receiver_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host_models", "record_window_check.cpp"), "-o", path])
    return path


def run(exe, lines):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.check_output([exe], input="\n".join(lines).encode(), timeout=120, env=env).decode().split("\n")[:-1]
    assert len(out) == len(lines)
    return [o.split("|") for o in out]


def record(tmp_path, size=SIZE):
    data = bytes((37 * i + 11) % 251 for i in range(size))
    path = tmp_path / "in.bin"
    path.write_bytes(data)
    return str(path), data


def test_have_and_the_byte_span_of_every_format(exe, tmp_path):
    path, _ = record(tmp_path)
    not_enough = "Could not read enough data from the data file (%d samples behind skipNumberOfBytes, %d wanted)"
    for fmt, bits in BITS.items():
        total = SIZE * 8 // bits
        for skip in (0, 3, total, total + 1):
            have = total - skip
            if fmt != PACKED:  # what the conditioners computed before the window existed
                assert have == SIZE // (bits // 8) - skip
            ns = [have, have + 1] if have >= 0 else [have, 0]
            got = run(exe, [f"O {path} {fmt} {skip}"] + [f"S {n}" for n in ns])
            assert got[0] == ["0", str(have), str(SIZE), ""], (fmt, skip)
            for n, g in zip(ns, got[1:]):
                if have < 0 or n > have:
                    assert g[0] == str(ERR_ARG) and g[4] == not_enough % (max(have, 0), n), (fmt, skip, n, g)
                else:
                    first, end = skip * bits // 8, -(-(skip + n) * bits // 8)
                    sub = skip & 1 if fmt == PACKED else 0
                    assert g == ["0", str(first), str(end), str(sub), ""], (fmt, skip, n, g)
                    assert end <= SIZE
    # a window of a part of the record: packed, from a high nibble to a low one
    got = run(exe, [f"O {path} {PACKED} 5", "S 8"])
    assert got[1] == ["0", "2", "7", "1", ""]  # samples 5 .. 12 lie in bytes 2 .. 6


def test_copy_through_in_chunks(exe, tmp_path):
    path, data = record(tmp_path)
    for span in (0, 5, 7, 20):
        dst = tmp_path / f"copy_{span}.bin"
        got = run(exe, [f"O {path} 0 0", "S 0", f"W {dst}", f"C 3 {3 + span} 7", "K"])
        assert [g[0] for g in got] == ["0"] * 5 and got[3] == ["0", ""] and got[4] == ["0", ""], (span, got)
        assert dst.read_bytes() == (b"\0" * 3 + data[3:3 + span] if span else b""), span
    whole = tmp_path / "copy_whole.bin"  # the default chunk, and two ranges with a gap the caller fills
    got = run(exe, [f"O {path} 1 2", "S 40", f"W {whole}", "C 0 4 0", "X 0 " + data[4:84].hex(), f"C 84 {SIZE} 0", "K"])
    assert [g[0] for g in got] == ["0"] * 7 and whole.read_bytes() == data
    kept = tmp_path / "copy_kept.bin"  # as the blanker calls it: lead = 3 and tail = 2 samples of the window are context
    got = run(exe, [f"O {path} 1 2", "S 40", f"W {kept}", "F 6", "X 6 " + data[10:80].hex(), "B 4", "K"])
    assert [g[0] for g in got] == ["0"] * 7 and kept.read_bytes() == data
    got = run(exe, [f"O {path} 0 0", "S 0", f"W {tmp_path / 'short.bin'}", f"C 90 {SIZE + 1} 7"])
    assert got[3] == [str(ERR_IO), f"short read of {path}"]


def test_read_and_write_at_the_ends_of_the_window(exe, tmp_path):
    path, data = record(tmp_path)
    dst = tmp_path / "out.bin"
    skip = 3
    first, end = 2 * skip, SIZE - 1  # s8c: 47 whole samples behind the skip, the file's odd last byte is no sample
    last = end - first - 1
    got = run(exe, [f"O {path} 1 {skip}", f"S {SIZE // 2 - skip}", f"W {dst}", "R 0 1", f"R {last} 1", f"R {last + 1} 1", f"R {last + 2} 1",
                    f"R 0 {last + 1}", "X 0 a5", f"X {last} 5a", "K"])
    assert got[1][:4] == ["0", str(first), str(end), "0"]
    assert got[3] == ["0", data[first:first + 1].hex(), ""] and got[4] == ["0", data[end - 1:end].hex(), ""]
    assert got[5] == ["0", data[end:end + 1].hex(), ""]  # (the byte behind this window is still the file's)
    assert got[6] == [str(ERR_IO), "", f"short read of {path}"]  # one byte past the file
    assert got[7] == ["0", data[first:end].hex(), ""]
    assert got[8] == ["0", ""] and got[9] == ["0", ""] and got[10] == ["0", ""]
    assert dst.read_bytes() == b"\0" * first + b"\xa5" + b"\0" * (last - 1) + b"\x5a"
    # a window that ends with the file: one byte past it is a short read
    got = run(exe, [f"O {path} 0 {skip}", f"S {SIZE - skip}", f"R {SIZE - skip - 1} 1", f"R {SIZE - skip} 1", f"R {SIZE - skip - 1} 2"])
    assert got[2] == ["0", data[-1:].hex(), ""]
    assert got[3] == [str(ERR_IO), "", f"short read of {path}"] and got[4] == [str(ERR_IO), "", f"short read of {path}"]


def test_names_and_files_that_are_not_there(exe, tmp_path):
    path, data = record(tmp_path)
    missing = str(tmp_path / "missing.bin")
    got = run(exe, [f"O {missing} 0 0"])
    assert got[0][0] == str(ERR_IO) and got[0][3] == f"Unable to read file {missing}"
    nowhere = str(tmp_path / "no_such_dir" / "never_written.bin")
    got = run(exe, [f"O {path} 0 0", "S 10", f"W {nowhere}"])
    assert got[2] == [str(ERR_IO), f"Unable to write file {nowhere}"]
    assert not os.path.exists(nowhere) and not os.path.exists(os.path.dirname(nowhere))
    got = run(exe, [f"N - {path} 1 0", f"N {path} - 1 0", f"N {path} - 0 0", f"N {path} {path} 1 0", f"N {path} {path} 0 0",
                    f"N {path} {missing} 1 -1", f"N {path} {missing} 1 0", f"N - - 0 -1"])
    assert got == [[str(ERR_ARG), "path_in or path_out is NULL"]] * 2 + [["0", ""], [str(ERR_ARG), "path_in and path_out are the same file"], ["0", ""],
                   [str(ERR_ARG), "skipNumberOfBytes < 0"], ["0", ""], [str(ERR_ARG), "path_in or path_out is NULL"]]
    # a window that is only read closes clean; an empty one is accepted
    got = run(exe, [f"O {path} 3 50", "S 0", "R 0 0", "K", "K"])
    assert got[0][:2] == ["0", "0"] and got[1] == ["0", "100", "100", "0", ""] and got[2] == ["0", "", ""] and got[3] == got[4] == ["0", ""]
    if os.path.exists("/dev/full"):  # an output that takes the bytes and cannot keep them: the failed fclose is a short write
        got = run(exe, [f"O {path} 0 0", "S 10", "W /dev/full", "X 0 0102", "K"])
        assert got[3] == ["0", ""] and got[4] == [str(ERR_IO), "short write on /dev/full"]
