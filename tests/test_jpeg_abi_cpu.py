"""CPU-only checks of the JPEG encoder's part of the C ABI (the pattern of
tests/test_abi_cpu.py): struct layouts, the exported function table bound from
plain C, and trik_hsv_jpeg_header (host code) against tests/jpeg_ref.py."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

import jpeg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_DIR = os.path.join(ROOT, "trik-media-sensors-dsp_amd", "trik_hsv")


@pytest.fixture(scope="module")
def abi():
    from trik_hsv import _abi

    return _abi


STRUCTS = ["TRIK_VIDTRANSCODE_CV_JPEG_InArgsAlg", "TRIK_VIDTRANSCODE_CV_JPEG_OutArgsAlg",
           "TRIK_VIDTRANSCODE_CV_JPEG_InArgs", "TRIK_VIDTRANSCODE_CV_JPEG_OutArgs"]
MIRRORS = ["JpegInArgsAlg", "JpegOutArgsAlg", "JpegInArgs", "JpegOutArgs"]


def test_jpeg_struct_layout_matches_c(abi):
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"trik_hsv.h\"\nint main(void){\n"
    for s in STRUCTS:
        prog += f'  printf("%zu\\n", sizeof({s}));\n'
    prog += '  printf("%zu %zu %zu\\n", offsetof(TRIK_VIDTRANSCODE_CV_JPEG_InArgsAlg, ifBlackAndWhite), ' \
            'offsetof(TRIK_VIDTRANSCODE_CV_JPEG_InArgs, alg), offsetof(TRIK_VIDTRANSCODE_CV_JPEG_OutArgs, alg));\n' \
            '  return 0;\n}\n'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "sz.c"), os.path.join(d, "sz")
        open(c, "w").write(prog)
        subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == 8 and out[1] == 4  # InArgs alg: uint8 + XDAS_Bool (int32); OutArgs alg: uint32
    for s, m, n in zip(STRUCTS, MIRRORS, out[:4]):
        assert C.sizeof(getattr(abi, m)) == n, (s, C.sizeof(getattr(abi, m)), n)
    assert out[4] == abi.JpegInArgsAlg.ifBlackAndWhite.offset == 4
    assert out[5] == abi.JpegInArgs.alg.offset and out[6] == abi.JpegOutArgs.alg.offset


XDAIS_PROG = r"""
#include <stdio.h>
#include "trik_hsv.h"
/* a Codec-Engine-style caller that binds only the function table */
int main(void) {
  const TRIK_IVIDTRANSCODE_Fxns* f = &TRIK_VIDTRANSCODE_CV_JPEG_FXNS;
  TRIK_IALG_MemRec m[16];
  TRIK_IALG_Fxns* parent = NULL;
  int n = f->ialg.algAlloc(NULL, &parent, m);
  if (n != 1 || m[0].size < sizeof(TRIK_IALG_Obj) || m[0].attrs != TRIK_IALG_PERSIST) return 10;
  if (f->ialg.implementationId != (const void*)f || !f->process || !f->control || !f->ialg.algInit ||
      !f->ialg.algFree || f->ialg.algActivate || f->ialg.algNumAlloc) return 20;
  if (f->process != TRIK_VIDTRANSCODE_CV_FXNS.process) return 30; /* one process() behind every table */
  unsigned char hd[608];
  if (trik_hsv_jpeg_header(50, 0, 640, 480, hd, (int32_t)sizeof hd) != 607 || hd[0] != 0xFF || hd[1] != 0xD8) return 40;
  if (trik_hsv_jpeg_header(50, 1, 640, 480, NULL, 0) != 324) return 41;
  /* a side SOF0 cannot hold: no header, an error message (checked here, in a process of its own, so that
     the library's last-error slot of the test process stays as the other tests expect it) */
  if (trik_hsv_jpeg_header(50, 0, 65536, 8, hd, (int32_t)sizeof hd) != 0 || !trik_hsv_last_error()[0]) return 42;
  if (trik_hsv_jpeg_header(50, 0, 8, -8, hd, (int32_t)sizeof hd) != 0) return 43;
  printf("%d %u\n", n, m[0].size);
  return 0;
}
"""


def test_jpeg_table_links_from_c_without_gpu():
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "x.c"), os.path.join(d, "x")
        open(c, "w").write(XDAIS_PROG)
        subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include')}", c,
                        f"-L{LIB_DIR}", "-ltrik_hsv", f"-Wl,-rpath,{LIB_DIR}", "-o", exe], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)


@pytest.mark.parametrize("bw", [False, True])
def test_jpeg_header_equals_the_reference(abi, bw):
    import trik_hsv

    for q in (0, 1, 10, 49, 50, 75, 100, 255):
        for w, h in ((32, 8), (640, 480), (320, 240), (65535, 65528)):
            assert trik_hsv.jpeg_header(q, bw, w, h) == jpeg_ref.header(q, bw, w, h), (q, w, h)
    lib = abi.load()
    buf = (C.c_uint8 * 700)(*([0x5A] * 700))
    n = 324 if bw else 607
    assert lib.trik_hsv_jpeg_header(50, int(bw), 64, 8, buf, n - 1) == n  # too small: the length alone
    assert all(b == 0x5A for b in buf)
    assert lib.trik_hsv_jpeg_header(50, int(bw), 64, 8, buf, n) == n
    assert bytes(buf[:n]) == jpeg_ref.header(50, bw, 64, 8) and all(b == 0x5A for b in buf[n:])
