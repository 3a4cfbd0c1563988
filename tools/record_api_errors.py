#!/usr/bin/env python3
"""Re-record tests/golden/api_errors.json, the calls the C ABI must refuse (tests/test_api_errors_cpu.py replays them).

    python tools/record_api_errors.py        (GECCO_HIP_LIB=<other build> records that library)

The fixture is the case list: rows of [symbol, args, return value, gecco_last_error() text or null].  This calls every row again and
rewrites the last two; a new case is a row [symbol, args, null, null] added by hand.  An argument is an int, a float or null; a pointer
argument takes an int too (4096 stands for "some device pointer": a case returns before the library launches, copies or dereferences
anything — a call that would need real memory behind a pointer to get past an earlier check is no case).  The one host structure an
entry point reads before it decides, the GeccoSplitJob table of the *_images_* calls, is a list of [W, img, Nout, K, ldw, transposed] rows.

Every GPU is hidden from the process first, and a case whose answer came from the HIP runtime is refused, so a mistaken row cannot
reach a device."""
import ctypes
import json
import os
import sys

os.environ["HIP_VISIBLE_DEVICES"] = ""   # (before the library, and with it the HIP runtime, is loaded)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gecco_amd import _lib   # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "api_errors.json")
PURE = ("_ok", "_ok_f16", "_bytes", "_tiles", "_index")   # queries: their return value is the whole answer


def main():
    lib = _lib.load()
    with open(FIXTURE) as f:
        cases = [row[:2] for row in json.load(f)]
    records = []
    for symbol, args in cases:
        restype, argtypes = _lib.SIGNATURES[symbol]
        assert len(args) == len(argtypes), (symbol, len(args), len(argtypes))
        rc = getattr(lib, symbol)(*[(_lib.GeccoSplitJob * len(a))(*[_lib.GeccoSplitJob(*r) for r in a]) if isinstance(a, list) else a for a in args])
        status = restype is ctypes.c_int and not symbol.endswith(PURE)
        message = lib.gecco_last_error().decode() if status and rc < 0 else None
        assert not (status and rc > 0) and "HIP error" not in (message or ""), f"{symbol}{args} got as far as the HIP runtime ({rc}): not a case"
        records.append([symbol, args, rc, message])
    with open(FIXTURE, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in records) + "\n]\n")
    print(f"{len(records)} cases ({sum(r[3] is not None for r in records)} refusals) -> {FIXTURE}")


if __name__ == "__main__":
    main()
