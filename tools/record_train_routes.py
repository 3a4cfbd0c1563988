"""Record tests/golden/train_routes.json: the library entry points every case of tests/_train_routes.py calls, in order.

Run it on the GPU from a checkout of the commit BEFORE a change to the training path's dispatch (with this file and
tests/_train_routes.py copied in if that commit predates them); tests/test_hip_train_routes.py then holds the change to it.

    python tools/record_train_routes.py [--out PATH]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests._train_routes import CASES, FIXTURE, run_case, save_fixture  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    routes = {}
    for name in CASES:
        routes[name] = run_case(name)
        print(f"{name}: {' + '.join(str(len(s)) for s in routes[name])} calls", flush=True)
    save_fixture(routes, args.out)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
