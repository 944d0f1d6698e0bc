"""The number set of the text-export tests (test_text_format.py on the host, test_gpu_text_export.py on
the device) and the expected bytes of the formatter: printf("%.{p}g") of the float as a double, which
Python's % operator computes exactly as glibc does, and the inf / nan spellings libstdc++ prints."""
import numpy as np


def bits(u):
    return np.asarray(u, np.uint32).view(np.float32)


SPECIALS = np.concatenate([
    np.array([0.0, -0.0, np.inf, -np.inf], np.float32),
    bits([0x7fc00000, 0xffc00000, 0x7f800001]),          # nan, -nan, a signalling nan
    np.array([1e-45, np.finfo(np.float32).max, 1e-4], np.float32),
    np.nextafter(np.float32(1e-4), np.float32(0)).reshape(1),
    np.array([1e16, 1e17, 9999995.0], np.float32)])


def number_set():
    rng = np.random.default_rng(20261019)
    parts = [bits(rng.integers(0, 2 ** 32, 2 ** 20, dtype=np.uint64).astype(np.uint32))]
    # every exponent field x {0, 1, all ones, eight random mantissas} x both signs
    man = np.concatenate([np.array([0, 1, 0x7fffff], np.uint32), rng.integers(0, 2 ** 23, 8).astype(np.uint32)])
    e = np.arange(256, dtype=np.uint32)
    for sign in (0, 1):
        parts.append(bits(((np.uint32(sign) << 31) | (e[:, None] << 23) | man[None, :]).reshape(-1)))
    # precision-17 ties: odd m / 2^18 in [0.1, 1) has exactly 18 significant digits, the last a 5
    m = np.arange(1, 2 ** 18, 2, dtype=np.int64)
    m = m[(m * 10 >= 2 ** 18)]
    assert len(m) == 117965
    parts.append((m / 2.0 ** 18).astype(np.float32))
    # precision-6 ties: k + 0.5 with six digits before the point
    parts.append((np.arange(100000, 1000000, 997) + 0.5).astype(np.float32))
    parts.append(np.array([100000.5, 100001.5, 999999.5], np.float32))
    parts.append(SPECIALS)
    return np.concatenate(parts)


def expected(x, precision):
    """The bytes the formatter must produce for every float32 of x."""
    fmt = "%%.%dg" % precision
    u = np.asarray(x, np.float32).view(np.uint32)
    out = []
    with np.errstate(invalid="ignore"):  # the signalling NaN
        wide = np.asarray(x, np.float32).astype(np.float64)
    for v, b in zip(wide.tolist(), u.tolist()):
        if b & 0x7f800000 == 0x7f800000:
            sign = "-" if b >> 31 else ""
            out.append((sign + ("nan" if b & 0x7fffff else "inf")).encode())
        else:
            out.append((fmt % v).encode())
    return out
