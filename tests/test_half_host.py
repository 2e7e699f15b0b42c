"""float16 / bfloat16 class-vector images (include/smesh_half.h), the part that needs no GPU: the extension header and its ctypes
table, dtype inference in the Python layer, the errors that need no device, and the numpy models of widening and narrowing that the
GPU tests compare the library with."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

from half_helpers import DTYPES, describe_rows, narrow, narrow_bf16, narrow_f16, random_probs16, subnormal_f16, widen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF_HEADER = os.path.join(ROOT, "include", "smesh_half.h")
HEADER = os.path.join(ROOT, "include", "smesh.h")
LIB = os.path.join(ROOT, "semantic_meshes_amd", "csrc", "libsmesh_hip.so")

C_CLIENT = r"""
#include "smesh_half.h"
#include <stddef.h>
/* what a C host writes: every entry point of the header, called with its declared argument types */
int use_half(smesh_renderer_t* r, smesh_aggregator_t* a, const smesh_camera_t* cams, const void* const* images,
             const float* const* weights, const void* indices, const float* f32, void* out16) {
  const int64_t strides[3] = {19 * 120, 19, 1};
  int s = smesh_fuse_view_probs16(r, a, &cams[0], images[0], SMESH_PROBS_F16, NULL, SMESH_MEM_DEVICE);
  if (s == SMESH_OK) s = smesh_fuse_views_probs16(r, a, cams, 8, images, SMESH_PROBS_BF16, weights, SMESH_MEM_HOST);
  if (s == SMESH_OK) s = smesh_aggregator_add_probs16(a, r, indices, SMESH_IDX_U32, NULL, SMESH_MEM_DEVICE, images[0], SMESH_PROBS_F16,
                                                      strides, SMESH_MEM_DEVICE, NULL, NULL, SMESH_MEM_HOST, 160, 120);
  if (s == SMESH_OK) s = smesh_narrow_probs(f32, out16, 1024, SMESH_PROBS_BF16, 0, SMESH_MEM_DEVICE);
  return s == SMESH_ERR_INVALID ? SMESH_PROBS_F32 : s;
}
"""


def _declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(smesh_[a-z0-9_]+)\s*\(", text)))


def test_extension_header_is_c99_and_the_library_exports_it(tmp_path):
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HALF_HEADER])
    src = tmp_path / "half_client.c"
    src.write_text(C_CLIENT)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-fsyntax-only", str(src)])
    from semantic_meshes_amd import _lib
    ext = _declared(HALF_HEADER)
    assert ext == sorted(["smesh_fuse_view_probs16", "smesh_fuse_views_probs16", "smesh_aggregator_add_probs16", "smesh_narrow_probs"])
    assert sorted(_lib.HALF_SIGNATURES) == ext
    assert sorted(_lib.SIGNATURES) == _declared(HEADER)            # the pinned ABI is what it was
    others = set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.VERTEX_SIGNATURES) | set(_lib.EVAL_SIGNATURES) | set(_lib.LABEL_IMAGE_SIGNATURES)
    assert not set(ext) & others
    exported = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    for name in ext:
        assert name in names, "%s is not exported by libsmesh_hip.so" % name
    codes = {k: int(v) for k, v in re.findall(r"#define\s+SMESH_PROBS_([A-Z0-9]+)\s+(\d+)", open(HALF_HEADER).read())}
    assert codes == {"F32": _lib.PROBS_F32, "F16": _lib.PROBS_F16, "BF16": _lib.PROBS_BF16} == {"F32": 0, "F16": 1, "BF16": 2}
    assert _lib.PROBS_NAMES == {0: "float32", 1: "float16", 2: "bfloat16"}


def test_the_entry_points_refuse_bad_dtype_codes_without_a_device():
    """The dtype is checked before anything touches a GPU: SMESH_PROBS_F32 and unknown codes are SMESH_ERR_INVALID, with a message."""
    from semantic_meshes_amd import _lib
    lib = _lib.lib()
    x, y = np.zeros(8, np.float32), np.zeros(8, np.uint16)
    for code in (_lib.PROBS_F32, 3, -1, 17):
        status = lib.smesh_narrow_probs(x.ctypes.data_as(ctypes.c_void_p), y.ctypes.data_as(ctypes.c_void_p), 8, code, 0, _lib.MEM_HOST)
        assert status == _lib.ERR_INVALID
        assert b"dtype" in lib.smesh_last_error() or b"PROBS" in lib.smesh_last_error()
        with pytest.raises(ValueError):
            _lib.check(status)
    assert _lib.get_option("half_max_classes") == 48
    assert _lib.get_option("last_fuse_probs_dtype") == 0


def test_dtype_inference():
    from semantic_meshes_amd import _lib, dlpack
    from semantic_meshes_amd.device import DeviceArray, describe
    from semantic_meshes_amd.fusion import probs_code
    img = np.zeros((4, 3, 5), np.float16)
    ptr, mem, shape, dt, strides, keep = describe(img, 3, "probs image")
    assert mem == _lib.MEM_HOST and probs_code(dt, keep) == _lib.PROBS_F16          # numpy float16
    assert probs_code(np.float32) == _lib.PROBS_F32
    assert probs_code(np.float64) is None and probs_code(np.int16) is None and probs_code(np.uint16) is None

    class Cai:      # a device array of another framework: __cuda_array_interface__ with typestr <f2
        __cuda_array_interface__ = {"shape": (4, 3, 5), "typestr": "<f2", "data": (0x1000, False), "version": 2, "strides": None}
    ptr, mem, shape, dt, strides, keep = describe(Cai(), 3, "probs image")
    assert mem == _lib.MEM_DEVICE and strides == (15, 5, 1) and probs_code(dt, keep) == _lib.PROBS_F16

    bits = np.arange(60, dtype=np.uint16).reshape(4, 3, 5)
    capsule = dlpack.to_capsule(bits.ctypes.data, bits.shape, (15, 5, 1), bits.dtype, dlpack.kDLCPU, 0, bits, bfloat16=True)
    ptr, mem, shape, dt, strides, keep = describe(capsule, 3, "probs image")        # DLPack kDLBfloat / 16
    assert mem == _lib.MEM_HOST and ptr == bits.ctypes.data and dt == np.uint16 and keep.bfloat16
    assert probs_code(dt, keep) == _lib.PROBS_BF16
    keep.close()
    plain = dlpack.Imported(dlpack.to_capsule(bits.ctypes.data, bits.shape, (15, 5, 1), bits.dtype, dlpack.kDLCPU, 0, bits))
    assert not plain.bfloat16 and probs_code(plain.dtype, plain) is None             # a uint16 tensor is no class-vector image
    plain.close()
    half = dlpack.Imported(dlpack.to_capsule(img.ctypes.data, img.shape, (15, 5, 1), img.dtype, dlpack.kDLCPU, 0, img))
    assert probs_code(half.dtype, half) == _lib.PROBS_F16                            # DLPack kDLFloat / 16
    half.close()

    class TorchLikeBf16:     # a bfloat16 tensor of another framework: the array interface cannot describe it and raises, DLPack can
        @property
        def __cuda_array_interface__(self):
            raise TypeError("Can't get __cuda_array_interface__ on a tensor of dtype bfloat16")

        def __dlpack__(self, stream=None):
            return dlpack.to_capsule(bits.ctypes.data, bits.shape, (15, 5, 1), bits.dtype, dlpack.kDLCPU, 0, bits, bfloat16=True)

        def __dlpack_device__(self):
            return (dlpack.kDLCPU, 0)
    ptr, mem, shape, dt, strides, keep = describe(TorchLikeBf16(), 3, "probs image")
    assert ptr == bits.ctypes.data and shape == (4, 3, 5) and strides == (15, 5, 1) and dt == np.uint16 and keep.bfloat16
    assert probs_code(dt, keep) == _lib.PROBS_BF16
    from semantic_meshes_amd.fusion import _peek_code
    assert _peek_code(TorchLikeBf16(), None) is None          # (not knowable without consuming a capsule: add_many lets add() decide)
    keep.close()

    assert probs_code(np.uint16, None, "bfloat16") == _lib.PROBS_BF16                # uint16 + keyword
    marked = DeviceArray(0x1000, (4, 3, 5), np.uint16)
    assert probs_code(marked.dtype, marked) is None
    marked.bfloat16 = True                                                           # what narrow_probs returns
    assert probs_code(marked.dtype, marked) == _lib.PROBS_BF16 and marked.transpose(1, 0, 2).bfloat16
    assert probs_code(np.float16, None, "float16") == _lib.PROBS_F16
    for dt, name in ((np.float16, "bfloat16"), (np.float32, "bfloat16"), (np.int16, "bfloat16"), (np.float32, "float16"),
                     (np.uint16, "float16"), (np.float16, "float32"), (np.float16, "int8")):
        with pytest.raises(ValueError):
            probs_code(dt, None, name)


def test_value_errors_that_need_no_device():
    """The Python layer refuses a wrong `probs_dtype` and mixed dtypes before any handle is used."""
    from semantic_meshes_amd import fusion

    class Agg(fusion._MeshAggregator):      # the methods under test, without a library handle
        def __init__(self):
            self.primitives, self.classes, self.device, self.defer, self._pending = 10, 5, 0, False, []

        def __del__(self):
            pass

    class Cam:
        resolution = (4, 3)
        _pod = fusion._lib.CameraPOD()

    agg, r = Agg(), types.SimpleNamespace(device=0, _h=None)
    f16, f32, u16 = np.zeros((4, 3, 5), np.float16), np.zeros((4, 3, 5), np.float32), np.zeros((4, 3, 5), np.uint16)
    idx = np.zeros((4, 3), np.uint32)
    for bad in (f16, f32):
        with pytest.raises(ValueError, match="bfloat16"):
            agg.add(idx, bad, probs_dtype="bfloat16")
        with pytest.raises(ValueError, match="bfloat16"):
            agg.fuse_view(r, Cam(), bad, probs_dtype="bfloat16")
        with pytest.raises(ValueError, match="bfloat16"):
            agg.fuse_views(r, [Cam()], [bad], probs_dtype="bfloat16")
    with pytest.raises(ValueError, match="one dtype"):
        agg.fuse_views(r, [Cam(), Cam()], [f16, f32])
    with pytest.raises(ValueError, match="one dtype"):
        agg.add_many([idx, idx], [f32, f16])
    with pytest.raises(ValueError):
        agg.fuse_view(r, Cam(), u16)          # uint16 without the keyword is no class-vector image
    with pytest.raises(ValueError):
        agg.fuse_views_ranged(r, [Cam()], [f16])


def test_widen_and_narrow_models_agree():
    """Narrow-then-widen is the identity on every representable value, for both formats; the bfloat16 rounding written out on the bits
    agrees with exact arithmetic on ties, subnormals and overflow; binary16 subnormals widen to value * 2^-24."""
    every = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    for dtype in DTYPES:
        w = widen(every, dtype)
        back = narrow(w, dtype)
        nan = np.isnan(w)
        assert np.array_equal(back[~nan], every[~nan])
        assert np.isnan(widen(back[nan], dtype)).all()
        assert np.array_equal(np.signbit(w), (every >> 15).astype(bool))
    sub = every[subnormal_f16(every)]
    assert len(sub) == 2 * 1023
    assert np.array_equal(np.abs(widen(sub, "float16")), (sub & 0x3FF).astype(np.float32) * np.float32(2.0 ** -24))
    assert np.array_equal(widen(np.array([0x0000, 0x8000, 0x7C00, 0xFC00], np.uint16), "float16").view(np.uint32),
                          np.array([0, 0x80000000, 0x7F800000, 0xFF800000], np.uint32))
    assert np.array_equal(widen(np.array([0x0000, 0x8000, 0x7F80, 0xFF80, 0x3F80], np.uint16), "bfloat16").view(np.uint32),
                          np.array([0, 0x80000000, 0x7F800000, 0xFF800000, 0x3F800000], np.uint32))
    # bfloat16 round to nearest even against float64 arithmetic: the nearest of the two neighbours, the even one on a tie
    rng = np.random.default_rng(5)
    x = rng.integers(0, 1 << 32, size=200_000, dtype=np.uint64).astype(np.uint32)
    x[:6] = [0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x7F7FFFFF, 0x00008000]     # ties down / up, either side, overflow, subnormal tie
    xf = x.view(np.float32)
    fin = np.isfinite(xf)
    got = narrow_bf16(xf)
    lo = (x >> 16).astype(np.uint16)                      # truncation: the neighbour towards zero
    hi = (lo.astype(np.uint32) + 1).astype(np.uint16)     # the next one away from zero (may be inf)
    with np.errstate(over="ignore", invalid="ignore"):
        vlo, vhi, v = widen(lo, "bfloat16").astype(np.float64), widen(hi, "bfloat16").astype(np.float64), xf.astype(np.float64)
        vhi = np.where(np.isinf(vhi), np.sign(vhi) * 2.0 ** 128, vhi)      # (IEEE: overflow rounds as if the exponent range went on)
        dlo, dhi = np.abs(v - vlo), np.abs(vhi - v)
    want = np.where(dlo < dhi, lo, np.where(dhi < dlo, hi, np.where(lo & 1, hi, lo)))
    assert np.array_equal(got[fin], want[fin])
    assert got[4] == 0x7F80 and got[0] == 0x3F80 and got[1] == 0x3F82                  # overflow to inf; ties to even
    assert np.isnan(widen(narrow_bf16(np.array([np.nan], np.float32)), "bfloat16")).all()
    assert np.array_equal(narrow_f16(np.array([65520.0, 65519.0, 2.0 ** -25, 2.0 ** -25 * 1.0001, 2.0 ** -24], np.float32)),
                          np.array([0x7C00, 0x7BFF, 0x0000, 0x0001, 0x0001], np.uint16))


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_test_images_hold_what_the_tests_need(dtype):
    rng = np.random.default_rng(1)
    img = random_probs16(rng, 160, 120, 19, dtype)
    zero, below, above, sub = describe_rows(img, dtype)
    assert 300 < zero < 900 and below > 50 and above > 50
    if dtype == "float16":
        assert sub > 1000
