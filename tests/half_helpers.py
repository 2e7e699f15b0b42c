"""numpy models of the 16-bit class-vector formats (include/smesh_half.h) for the tests: the exact widening that defines the
feature, round-to-nearest-even narrowing, and the test images.  Images travel as uint16 BIT PATTERNS for both formats (numpy has no
bfloat16); `typed()` gives the array a user would hand to the library."""
import numpy as np

DTYPES = ("float16", "bfloat16")


def widen(bits16, dtype):
    """uint16 bit patterns -> float32, exactly: binary16 -> binary32 (subnormals kept) / the bits moved to the upper half."""
    bits16 = np.asarray(bits16)
    assert bits16.dtype == np.uint16
    if dtype == "float16":
        return bits16.view(np.float16).astype(np.float32)
    return (bits16.astype(np.uint32) << np.uint32(16)).view(np.float32)


def narrow_bf16(x):
    """float32 -> bfloat16 bit patterns, round to nearest, ties to even, written out on the bits: add half an ulp of the result
    (0x7FFF) plus the result's last bit, keep the upper half.  Overflow carries into the exponent and gives inf; a NaN stays one."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    rounded = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)
    nan = (u & np.uint64(0x7FFFFFFF)) > np.uint64(0x7F800000)
    return np.where(nan, (u >> np.uint64(16)) | np.uint64(0x40), rounded).astype(np.uint16)


def narrow_f16(x):
    """float32 -> binary16 bit patterns by numpy's conversion (IEEE round to nearest even, overflow to inf, subnormals kept)."""
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(x, dtype=np.float32).astype(np.float16).view(np.uint16)


def narrow(x, dtype):
    return narrow_f16(x) if dtype == "float16" else narrow_bf16(x)


def typed(bits16, dtype):
    """What a user passes: a float16 array, or uint16 bits (with probs_dtype="bfloat16")."""
    return bits16.view(np.float16) if dtype == "float16" else bits16


def kw(dtype):
    return {"probs_dtype": "bfloat16"} if dtype == "bfloat16" else {}


def subnormal_f16(bits16):
    """Elements that are binary16 subnormals (exponent field 0, mantissa not 0)."""
    return ((bits16 & 0x7C00) == 0) & ((bits16 & 0x03FF) != 0)


def random_probs16(rng, W, H, C, dtype):
    """(W,H,C) uint16 bit patterns of softmax rows narrowed to `dtype`: about 3 % all-zero don't-care rows, about 4 % rows scaled so
    that their widened sum lies just below or just above 0.5 (the `sum > 0.5f` test of Mesh.h:98 sees both sides), and -- from 19
    classes on -- many elements below 6.1e-5, which are binary16 subnormals."""
    logits = rng.normal(0.0, 5.0, size=(W, H, C)).astype(np.float32)
    e = np.exp(logits - logits.max(axis=-1, keepdims=True))
    p = (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)
    u = rng.random((W, H))
    p[u < 0.03] = 0.0
    edge = (u >= 0.03) & (u < 0.07)
    p[edge] *= rng.choice(np.array([0.49, 0.4995, 0.5005, 0.51], np.float32), size=int(edge.sum()))[:, None]
    return narrow(p, dtype)


def describe_rows(bits16, dtype):
    """(all-zero rows, rows with 0 < sum <= 0.5, rows with 0.5 < sum < 0.52, binary16-subnormal elements) of an image: what the tests
    assert their data contains.  The sum is the float32 sequential one of the spec."""
    w = widen(bits16, dtype)
    s = np.zeros(w.shape[:-1], np.float32)
    for c in range(w.shape[-1]):
        s = s + w[..., c]
    sub = int(subnormal_f16(bits16).sum()) if dtype == "float16" else 0
    return int((s == 0).sum()), int(((s > 0) & (s <= 0.5)).sum()), int(((s > 0.5) & (s < 0.52)).sum()), sub
