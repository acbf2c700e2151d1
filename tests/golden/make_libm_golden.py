"""Writes tests/golden/libm_expm1_log1p.json: arguments and results of the C library's expm1 and log1p (through
math.expm1 / math.log1p) as hex floats, on the arguments the exact log-MAP demapper can produce.  Run it on a
machine with glibc 2.35 (the file records platform.libc_ver()); the tests hold the package's NumPy restatement of
the two algorithms (channel/libm_np.py) to this file bit for bit, and skip their live half where the machine's own
math.* does not reproduce it.

expm1: q from -0.0 down through the branch boundaries of s_expm1.c -- 2^-54 (x itself), 0.5 ln 2 and 1.5 ln 2
(the argument reduction), every k ln 2 +- 0.5 ln 2 turn of the reduction's k down to -56, -37.43 = -54 ln 2, the
constant from 56 ln 2 on -- to -inf.  log1p: [0, 7] with 0.0, 2^-54, 2^-29, the sqrt(2) - 1 boundary, the turns of
k at 2^j sqrt(2) - 1, and 2^j - 1 (f == 0)."""
import json
import math
import os
import platform
import struct

import numpy as np


def around(x, n=12):
    """x and n doubles to either side of it"""
    out, lo, hi = [x], x, x
    for _ in range(n):
        lo, hi = math.nextafter(lo, -math.inf), math.nextafter(hi, math.inf)
        out += [lo, hi]
    return out


def short_hex(v):
    """float.hex without the mantissa's trailing zeros (float.fromhex reads it back exactly)"""
    h = float(v).hex()
    if "." not in h:
        return h
    head, exp = h.split("p")
    head = head.rstrip("0")
    return (head + "0" if head.endswith(".") else head) + "p" + exp


def from_hi(hi_word):
    return struct.unpack("<d", struct.pack("<Q", hi_word << 32))[0]


def main():
    rng = np.random.default_rng(20261021)
    ln2 = math.log(2.0)
    ex = [-0.0, -5e-324, -2.2250738585072014e-308, -math.inf, -1.7976931348623157e308, -1e300, -745.2, -709.8, -100.0]
    for hw in (0x3C900000, 0x3FD62E42, 0x3FD62E43, 0x3FF0A2B2, 0x4043687A, 0x40862E42):
        ex += [-v for v in around(from_hi(hw))]
    for k in range(1, 58):
        ex += [-v for v in around((k + 0.5) * ln2, 2)] + [-k * ln2, -float(k)]
    ex += [-v for v in around(54 * ln2)] + [-37.43]
    ex += (-np.exp(rng.uniform(math.log(2.0 ** -60), math.log(60.0), 120))).tolist()
    ex += (-rng.uniform(0.0, 40.0, 80)).tolist()
    ex = [v for v in ex if v <= 0.0]
    lg = [0.0, 5e-324, 0.5, 1.0, 3.0, 7.0, 2.0, 4.0, 6.0, 5.0]
    for hw in (0x3C900000, 0x3E200000, 0x3FDA827A):
        lg += around(from_hi(hw))
    for j in (1, 2, 4):
        lg += around(j * math.sqrt(2.0) - 1.0, 6) + around(2.0 * j - 1.0, 6)
    lg += np.exp(rng.uniform(math.log(2.0 ** -60), math.log(7.0), 150)).tolist()
    lg += rng.uniform(0.0, 7.0, 150).tolist()
    lg = [v for v in lg if 0.0 <= v <= 7.0]
    doc = {"libc": list(platform.libc_ver()),
           "expm1": [[short_hex(a), short_hex(math.expm1(a))] for a in ex],
           "log1p": [[short_hex(a), short_hex(math.log1p(a))] for a in lg]}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libm_expm1_log1p.json")
    with open(path, "w") as f:  # eight pairs a line: a file of a few hundred lines
        f.write('{"libc": %s' % json.dumps(doc["libc"]))
        for name in ("expm1", "log1p"):
            rows = [", ".join(json.dumps(p) for p in doc[name][i:i + 8]) for i in range(0, len(doc[name]), 8)]
            f.write(',\n"%s": [\n%s\n]' % (name, ",\n".join(rows)))
        f.write("}\n")
    print(path, len(ex), len(lg))


if __name__ == "__main__":
    main()
