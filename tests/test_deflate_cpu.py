"""The block deflate encoder, CPU side (include/dmslam_io.h: dms_deflate_blocks over csrc/deflate_core.hpp, the code the device
encoder compiles too): every case of tests/deflate_cases.py must inflate, with Python's zlib, to the input, as one correctly ended
stream within the bound; the bench's depth frame must come out smaller than a Huffman-only zlib stream of it; and the per-block
stages, run in reverse block order under the sanitizers (tests/deflate_host.cpp), must give the sequential encoder's bytes."""
import os
import shutil
import subprocess
import zlib

import pytest

from tests import deflate_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ing():
    from densemonoslam_amd import ingest

    return ingest


def test_cases_cover_what_the_encoder_can_go_wrong_on(ing):
    B = dc.block_size()
    assert 256 <= B <= 32768
    lens = {name: len(x) for name, x in dc.cases()}
    for n in (1, 2, 3, 4, B - 1, B, B + 1, 3 * B + 17, 257, 258, 259, 260, 2 * B + 5, 40000, 160 * 120 * 2, 64 * 48 * 2, 640 * 480 * 2):
        assert n in lens.values(), n
    assert lens["zeros_70001"] > 65535 and lens["repeat_at_32768"] == lens["repeat_at_32769"] == 40000
    a, b = dc.by_name("repeat_at_32768"), dc.by_name("repeat_at_32769")
    assert a[32768:] == a[:40000 - 32768] and b[32769:] == b[:40000 - 32769] and b[32768:] != b[:40000 - 32768]
    x = dc.by_name("all_distinct")
    assert len({x[i:i + 3] for i in range(len(x) - 2)}) == len(x) - 2
    assert len(set(dc.by_name("skewed_21_values"))) >= 19


def test_every_case_inflates_to_the_input_as_one_stream_within_the_bound(ing):
    for name, x in dc.cases():
        z = ing.deflate_blocks(x)
        assert zlib.decompress(z) == x, name
        assert len(z) <= ing.deflate_blocks_bound(len(x)), name
        o = zlib.decompressobj()
        assert o.decompress(z) == x and o.eof and o.unused_data == b"", name  # one stream, correctly ended, Adler-32 right
        assert z[:2] == b"\x78\x01" and int.from_bytes(z[:2], "big") % 31 == 0
        assert int.from_bytes(z[-4:], "big") == zlib.adler32(x), name
        assert ing.deflate_blocks(x) == z, name  # the same bytes on every run


def test_kinds_of_block(ing):
    """incompressible input is stored: B bytes grow by 5; a run costs a few bytes; a literal-only block carries the one-code
    distance tree and is still smaller than fixed codes would make it"""
    B = dc.block_size()
    assert len(ing.deflate_blocks(dc.by_name("random_B"))) == B + 5 + 6
    x = dc.by_name("random_3B+17")
    assert len(x) + 5 * 3 + 6 < len(ing.deflate_blocks(x)) <= len(x) + 5 * 4 + 6  # the 17 bytes behind may be cheaper with fixed codes
    assert len(ing.deflate_blocks(dc.by_name("run_258"))) < 20 and len(ing.deflate_blocks(dc.by_name("zeros_70001"))) < 70001 // 100
    x = dc.by_name("all_distinct")
    fixed = zlib.compressobj(9, zlib.DEFLATED, 15, 9, zlib.Z_FIXED)
    assert len(ing.deflate_blocks(x)) < len(fixed.compress(x) + fixed.flush())
    # the match at distance 32 768 is used, the one at 32 769 cannot be
    assert len(ing.deflate_blocks(dc.by_name("repeat_at_32768"))) + 4000 < len(ing.deflate_blocks(dc.by_name("repeat_at_32769")))
    assert len(ing.deflate_blocks(dc.by_name("rows_1280"))) < 25600 // 8  # rows that repeat the row above, across block edges


def test_size_of_the_bound(ing):
    for n in (4096, 4097, 5000, 65536, 614400, 1 << 20, (1 << 24) + 3, 1 << 31):
        assert ing.deflate_blocks_bound(n) <= n + n // 256 + 64, n
    assert ing.deflate_blocks_bound(1) >= 1 + 5 + 6


def test_refusals(ing):
    from densemonoslam_amd.capi import DmsError, lib

    with pytest.raises(DmsError) as e:
        ing.deflate_blocks(b"")
    assert e.value.code == -1
    x = dc.by_name("rows_1280")
    bound = ing.deflate_blocks_bound(len(x))
    for cap in (0, bound - 1):
        with pytest.raises(DmsError, match="needed") as e:
            ing.deflate_blocks(x, cap=cap)
        assert e.value.code == ing.DMS_ERR_CAPACITY and ing.deflate_blocks.last_written == bound
    assert zlib.decompress(ing.deflate_blocks(x, cap=bound)) == x
    out = ing.C.create_string_buffer(64)
    w = ing.C.c_size_t(0)
    assert lib.dms_deflate_blocks(None, 4, out, 64, ing.C.byref(w)) == -1 and lib.dms_deflate_blocks(b"abcd", 4, None, 64, ing.C.byref(w)) == -1
    assert lib.dms_deflate_blocks(b"abcd", 4, out, 64, None) == -1


def test_bench_frame_is_smaller_than_huffman_only(ing):
    """dynamic tables without a working matcher, or fixed tables, cannot pass; the ratio to zlib level 1 (the reference's
    converters' setting) is printed for DESIGN 2.10, not asserted"""
    x = dc.by_name(dc.VGA)
    z = ing.deflate_blocks(x)
    h = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_HUFFMAN_ONLY)
    huffman_only = len(h.compress(x) + h.flush())
    level1, level6 = len(zlib.compress(x, 1)), len(zlib.compress(x, 6))
    print("deflate_blocks %d bytes; zlib level 1 %d (ratio %.3f), default level %d (ratio %.3f), Huffman only %d" %
          (len(z), level1, len(z) / level1, level6, len(z) / level6, huffman_only))
    assert len(z) < huffman_only


def test_header_declares_the_block_encoder_in_plain_c(ing, tmp_path):
    src = tmp_path / "abi_check.c"
    src.write_text('#include "dmslam_io_write.h"\n'
                   "int main(void) { dms_deflate_dev* d = 0; size_t n = dms_deflate_blocks_bound(1); (void)d; (void)n;\n"
                   "  return DMS_RECORD_DEFAULT_DEPTH_ON_DEVICE; }\n")
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", inc, "-fsyntax-only", str(src)])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", inc, "-fsyntax-only", "-x", "c++", str(src)])
    from densemonoslam_amd import capi

    for n in ("dms_deflate_blocks_block_size", "dms_deflate_blocks_bound", "dms_deflate_blocks", "dms_deflate_dev_create", "dms_deflate_dev_destroy",
              "dms_deflate_dev_encode", "dms_deflate_dev_result", "dms_deflate_dev_result_at", "dms_jpeg_enc_set_depth_on_device"):
        assert hasattr(capi.lib, n), n
    assert capi.lib.dms_deflate_dev_create(None, 1000, 2) == -1  # argument validation happens before any device access
    hdr = open(os.path.join(inc, "dmslam_io_write.h")).read()
    assert "#define DMS_RECORD_DEFAULT_DEPTH_ON_DEVICE %d" % ing.RECORD_DEFAULT_DEPTH_ON_DEVICE in hdr


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_blocks_in_reverse_order_equal_the_sequential_encoder_under_the_sanitizers(ing, tmp_path):
    """tests/deflate_host.cpp: the code builder on crafted counts, then every case through the per-block stages; here: exit 0, no
    sanitizer report, one line a case, and the program's bytes are the library's"""
    exe = str(tmp_path / "deflate_host")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + ROOT, os.path.join(ROOT, "tests", "deflate_host.cpp"), "-o", exe])
    args = []
    for name, x in dc.cases():
        f = tmp_path / (name + ".bin")
        f.write_bytes(x)
        args += [name, str(f)]
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and not out.stderr.strip(), (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    lines = out.stdout.splitlines()
    assert lines[0] == "codes ok" and len(lines) == 1 + len(dc.cases()) and all(l.endswith(" ok") for l in lines), out.stdout
    by = {l.split()[0]: l.split() for l in lines[1:]}
    for name, x in dc.cases():
        assert int(by[name][1]) == (len(x) + dc.block_size() - 1) // dc.block_size() and int(by[name][2]) == len(ing.deflate_blocks(x)), name
