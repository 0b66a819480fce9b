"""CPU-only checks of the ov7670 MxN colour-grid sensor's ABI and of the test
reference itself (tests/mxn_ref.py): the four new structs have the C layout,
the exported function table binds from plain C, the host-built colour table
equals the reference's HSVtoRGB on all 512 bins (the library loads and
trik_hsv_mxn_color runs without a GPU), and the order-free winner rule the
kernel implements equals the reference's sequential loop."""
import ctypes as C
import os
import random
import subprocess
import tempfile

import mxn_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRUCTS = [("TRIK_VIDTRANSCODE_CV_MXN_InArgsAlg", "MxnInArgsAlg"), ("TRIK_VIDTRANSCODE_CV_MXN_InArgs", "MxnInArgs"),
           ("TRIK_VIDTRANSCODE_CV_MXN_OutArgsAlg", "MxnOutArgsAlg"), ("TRIK_VIDTRANSCODE_CV_MXN_OutArgs", "MxnOutArgs")]
FIELDS = [("TRIK_VIDTRANSCODE_CV_MXN_InArgsAlg", "MxnInArgsAlg", "widthM"),
          ("TRIK_VIDTRANSCODE_CV_MXN_InArgsAlg", "MxnInArgsAlg", "heightN"),
          ("TRIK_VIDTRANSCODE_CV_MXN_InArgs", "MxnInArgs", "alg"),
          ("TRIK_VIDTRANSCODE_CV_MXN_OutArgsAlg", "MxnOutArgsAlg", "outColor"),
          ("TRIK_VIDTRANSCODE_CV_MXN_OutArgs", "MxnOutArgs", "alg")]


def test_mxn_struct_layout_matches_c():
    from trik_hsv import _abi

    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "trik_hsv.h"\nint main(void){\n'
    for s, _ in STRUCTS:
        prog += f'  printf("%zu\\n", sizeof({s}));\n'
    for s, _, f in FIELDS:
        prog += f'  printf("%zu\\n", offsetof({s}, {f}));\n'
    prog += "  return 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "sz.c"), os.path.join(d, "sz")
        open(c, "w").write(prog)
        subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    for (s, m), n in zip(STRUCTS, out):
        assert C.sizeof(getattr(_abi, m)) == n, (s, n)
    for (s, m, f), n in zip(FIELDS, out[len(STRUCTS):]):
        assert getattr(getattr(_abi, m), f).offset == n, (s, f, n)
    assert out[1] == 20 and out[2] == 400  # InArgs, OutArgsAlg
    assert out[3] == C.sizeof(_abi.IVidtranscodeOutArgs) + 400


XDAIS_PROG = r"""
#include <stdio.h>
#include "trik_hsv.h"
int main(void) {
  const TRIK_IVIDTRANSCODE_Fxns* f = &TRIK_VIDTRANSCODE_CV_MXN_FXNS;
  TRIK_IALG_MemRec m[16];
  TRIK_IALG_Fxns* parent = NULL;
  int n = f->ialg.algAlloc(NULL, &parent, m);
  if (n != 1 || m[0].size < sizeof(TRIK_IALG_Obj) || m[0].attrs != TRIK_IALG_PERSIST) return 10;
  if (f->ialg.implementationId != (const void*)f || !f->process || !f->control || !f->ialg.algInit ||
      !f->ialg.algFree) return 20;
  if (f->ialg.algInit == TRIK_VIDTRANSCODE_CV_OV7670_FXNS.ialg.algInit) return 30;
  printf("%u\n", trik_hsv_mxn_color(0, 3, 3));
  return 0;
}
"""


def test_mxn_table_links_from_c_without_gpu():
    lib_dir = os.path.join(ROOT, "trik-media-sensors-dsp_amd", "trik_hsv")
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "x.c"), os.path.join(d, "x")
        open(c, "w").write(XDAIS_PROG)
        subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include')}", c,
                        f"-L{lib_dir}", "-ltrik_hsv", f"-Wl,-rpath,{lib_dir}", "-o", exe], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert int(r.stdout) == mxn_ref.hsv_to_rgb(0, 192, 192)


def test_mxn_color_table_equals_reference():
    """All 512 entries of the host-built table (no GPU call is made)."""
    from trik_hsv import _abi

    lib = _abi.load()
    for h in range(32):
        for s in range(4):
            for v in range(4):
                assert lib.trik_hsv_mxn_color(h, s, v) == mxn_ref.hsv_to_rgb(8 * h, 64 * s, 64 * v), (h, s, v)
    assert lib.trik_hsv_mxn_color(0, 0, 0) == 0
    for bad in ((-1, 0, 0), (32, 0, 0), (0, 4, 0), (0, 0, -1)):
        assert lib.trik_hsv_mxn_color(*bad) == 0


def test_mxn_color_known_values():
    """Hand-worked entries: below the value or saturation threshold, and hues
    where f * s is inexact (a fused multiply-add would change them)."""
    assert mxn_ref.hsv_to_rgb(0, 0, 0) == 0
    assert mxn_ref.hsv_to_rgb(80, 192, 0) == 0                # v = 0 < 0.2: black whatever the hue
    assert mxn_ref.hsv_to_rgb(80, 0, 192) == 0xC0C0C0         # s = 0: grey, int(192/255 * 255) = 192
    assert mxn_ref.hsv_to_rgb(0, 192, 192) == 0xC00000        # hue 0: r = v, g = t = 0, b = p = 0
    assert mxn_ref.hsv_to_rgb(0, 64, 128) == 0x800000         # s = 64/255 >= 0.2 counts as 1


def test_order_free_rule_equals_sequential_loop():
    """200 random small cells drawn from 3 bins (ties are common): the rule the
    kernel implements picks the sequential loop's winner."""
    rng = random.Random(20240611)
    ties = 0
    for _ in range(200):
        bins = rng.sample(range(mxn_ref.N_BINS), 3)
        cell = [rng.choice(bins) for _ in range(rng.randint(0, 12))]
        assert mxn_ref.winner_order_free(cell) == mxn_ref.winner_sequential(cell), cell
        ties += len(mxn_ref.tied_bins(cell)) >= 2
    assert ties >= 20  # at least one cell in ten is decided by the tie rule


def test_order_free_rule_named_cases():
    seq, free = mxn_ref.winner_sequential, mxn_ref.winner_order_free
    assert seq([]) == free([]) == 0
    assert seq([5, 9, 9, 5]) == free([5, 9, 9, 5]) == 9      # 9 reaches 2 first
    assert seq([9, 5, 5, 9]) == free([9, 5, 5, 9]) == 5
    assert seq([7, 3, 9, 3, 9, 7]) == free([7, 3, 9, 3, 9, 7]) == 3  # neither the first nor the last to appear
