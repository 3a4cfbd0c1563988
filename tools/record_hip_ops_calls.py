"""Record tests/golden/hip_ops_calls.json: what every case of tests/_hip_ops_calls.py hands the library, and the digests of its results.

Run it on the GPU from a checkout of the commit BEFORE a change to gecco_amd.hip_ops (with this file and tests/_hip_ops_calls.py
copied in if that commit predates them); tests/test_hip_ops_calls.py then holds the change to it.  Every case runs twice, the
second time with other bytes in the allocator's free blocks: a case whose two runs differ in their results keeps its call
record and gets "digest": null (named on the last line of the output).

    python tools/record_hip_ops_calls.py [--out PATH]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from tests._hip_ops_calls import CASES, FIXTURE, run_case, save_fixture  # noqa: E402


def scribble(byte: int) -> None:
    """Leave `byte` in free blocks of the caching allocator (sizes 512 B .. 64 MiB): what a later torch.empty hands out."""
    held = [torch.empty(512 << k, dtype=torch.uint8, device="cuda").fill_(byte) for k in range(18) for _ in range(3)]
    torch.cuda.synchronize()
    del held


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    records, unstable, t0 = {}, [], time.time()
    for name in CASES:
        scribble(0x00)
        first = run_case(name)
        scribble(0xFF)
        second = run_case(name)
        assert first["calls"] == second["calls"], f"{name}: the two runs made different calls"
        if first["digest"] != second["digest"]:
            unstable.append(name)
            first["digest"] = None
        records[name] = first
        raised = [c for c in first["calls"] if isinstance(c, str)]
        print(f"{name}: {len(first['calls'])} calls, {len(first['digest'] or [])} tensors" + (f"  {raised[0]}" if raised else ""), flush=True)
    save_fixture(records, args.out)
    print(f"wrote {args.out}: {len(records)} cases in {time.time() - t0:.1f} s (two runs each)")
    print(f"{len(unstable)} cases with results that differ between two runs: {unstable}")


if __name__ == "__main__":
    main()
