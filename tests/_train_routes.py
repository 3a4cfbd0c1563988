"""Which library entry points a training step calls, in order: the cases and the recorder shared by
tests/test_hip_train_routes.py (asserts the sequences) and tools/record_train_routes.py (writes tests/golden/train_routes.json).

Every library call of the training path reports its name to `_lib.check`; a case's route is the list of those names over a forward and
a backward.  The cases are the smallest that reach every branch of the route predicates (gecco_amd/autograd/_routes.py): a 2-layer
LinearLift of feature_dim 128, 8 heads, 64 inducers, batch 2, at N = 128 (whole 128-row blocks: the A-stationary, h8 and fp16-tensor
routes), N = 96 (% 32 but not % 128: the LDS-DMA routes) and N = 100 (neither: the general GEMM), under each module default precision
with and without torch.autocast(float16); the switches that take a route away, one at a time, on the N = 128 autocast case; and the
smallest conditional model, for the lookup and ConvNeXt Functions.  Two steps per case: the second takes the recorded-image path."""
import contextlib
import difflib
import json
import os

import numpy as np
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_routes.json")
D, L, B, HW = 128, 2, 2, 64
OFF_SWITCHES = ("GECCO_TRAIN_IO16", "GECCO_TRAIN_A16", "GECCO_TRAIN_ACTBWD", "GECCO_TRAIN_INPROJ_SPLIT", "GECCO_WEIGHT_IMAGES")


def _cases() -> dict:
    out = {}
    for N in (128, 96, 100):
        for precision in ("fp32", "bf16x3", "mixed"):
            for autocast in (False, True):
                out[f"uncond-N{N}-{precision}" + ("-autocast" if autocast else "")] = dict(N=N, precision=precision, autocast=autocast)
    for name in OFF_SWITCHES:
        out[f"uncond-N128-mixed-autocast-{name}=0"] = dict(N=128, precision="mixed", autocast=True, env={name: "0"})
    out["cond-N128-bf16x3"] = dict(N=128, precision="bf16x3", autocast=False, cond=True)
    return out


CASES = _cases()


# The fixture.  Most routes differ from another in a few calls, so the file holds each distinct route once, as a list of pieces:
# a string of names separated by blanks ("raised: ..." stands alone), or [route, i, j] = the calls i .. j - 1 of an earlier route.
#   {"cases": {case: [route of step 1, route of step 2]}, "routes": {route: [piece, ...]}}
def load_fixture(path: str = FIXTURE) -> dict:
    """case -> [[names of step 1], [names of step 2]]"""
    with open(path) as f:
        doc = json.load(f)
    routes = {}
    for rid, pieces in doc["routes"].items():   # (in the file's order: a piece refers to a route before it)
        calls = []
        for p in pieces:
            calls += routes[p[0]][p[1]:p[2]] if isinstance(p, list) else [p] if p.startswith("raised: ") else p.split()
        routes[rid] = calls
    return {case: [routes[rid] for rid in rids] for case, rids in doc["cases"].items()}


def save_fixture(by_case: dict, path: str = FIXTURE) -> None:
    routes, ids, cases = {}, {}, {}   # routes: id -> pieces; ids: tuple of calls -> id
    for case, steps in by_case.items():
        cases[case] = []
        for calls in steps:
            key = tuple(calls)
            if key not in ids:
                base = max(ids, key=lambda b: difflib.SequenceMatcher(None, b, key, autojunk=False).ratio(), default=())
                pieces = []
                for tag, i, j, k, m in difflib.SequenceMatcher(None, base, key, autojunk=False).get_opcodes():
                    if tag == "equal" and j - i >= 4:
                        pieces.append([ids[base], i, j])
                        continue
                    names = [c for c in key[k:m] if not c.startswith("raised: ")]
                    pieces += [" ".join(names[n:n + 6]) for n in range(0, len(names), 6)] + [c for c in key[k:m] if c.startswith("raised: ")]
                ids[key] = f"r{len(ids):02d}"
                routes[ids[key]] = pieces
            cases[case].append(ids[key])
    with open(path, "w") as f:   # one case, one piece per line
        f.write('{"cases": {\n' + ",\n".join(f" {json.dumps(c)}: {json.dumps(r)}" for c, r in cases.items()) + '\n},\n"routes": {\n')
        f.write(",\n".join(f' "{rid}": [\n' + ",\n".join("  " + json.dumps(p) for p in ps) + "\n ]" for rid, ps in routes.items()) + "\n}}\n")


@contextlib.contextmanager
def recorded_calls():
    """The names `_lib.check` is called with while the block runs (hip_ops holds the function under a name of its own)."""
    from gecco_amd import _lib, hip_ops
    calls, orig = [], _lib.check

    def check(rc, what=""):
        calls.append(what)
        return orig(rc, what)
    _lib.check = hip_ops.check = check
    try:
        yield calls
    finally:
        _lib.check = hip_ops.check = orig


@contextlib.contextmanager
def _environment(env: dict):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _model_and_batch(case: dict):
    from gecco_amd.structs import Context3d, Example
    from oracle import cases, weights
    from tests.test_modules_cpu import build_cond, build_uncond, uncond_state_dict
    rs = np.random.RandomState(3)
    data = torch.from_numpy((0.5 * rs.randn(B, case["N"], 3)).astype(np.float32))
    if not case.get("cond"):
        m = build_uncond(D, L)
        m.load_state_dict(uncond_state_dict(weights.linear_lift_state_dict(11, D, L, cases.I, cases.H)), strict=True)
        return m.cuda().train(), Example(data.cuda(), None)
    # (as tests/test_hip_convnext.py::test_conditional_training_step_reaches_the_conditioner: a trainable ConvNeXt conditioner)
    from gecco_amd.models.feature_pyramid import ConvNeXtExtractor
    from tests.test_hip_convnext import _seeded_state
    cn = ConvNeXtExtractor(n_stages=3, model="tiny", pretrained=False)
    csd = _seeded_state(cn, 9)
    m = build_cond(D, L, conditioner=cn)
    p = weights.ray_network_state_dict(17, D, L, cases.I, cases.H)
    sd = {"backbone.model." + k: v for k, v in p.items()}
    sd["reparam.uvl_mean"], sd["reparam.uvl_std"] = p["reparam.uvl_mean"], p["reparam.uvl_std"]
    sd.update({"conditioner." + k: v for k, v in csd.items()})
    m.load_state_dict(sd, strict=True)
    img = torch.from_numpy(rs.rand(B, 3, HW, HW).astype(np.float32))
    _, K = weights.synthetic_context(4, B, hw=HW)
    return m.cuda().train(), Example(data.cuda(), Context3d(image=img.cuda(), K=K.cuda()))


def run_case(name: str, on_step=None, steps: int = 2) -> list:
    """The route of every step of the case: [[names of step 1], [names of step 2]].  on_step(step, loss, model), if given, is called
    after each step's backward (the gradients are in place).  A step in which an entry point refuses its arguments is part of the
    record as well: its route ends with "raised: <the error>", and the case ends with it."""
    from gecco_amd import _lib, hip_ops
    from gecco_amd import autograd as ag
    case = CASES[name]
    prev = hip_ops.default_precision()
    hip_ops.set_default_precision(case["precision"])
    ag.WEIGHT_IMAGES.__init__()
    routes = []
    try:
        with _environment(case.get("env", {})):
            m, batch = _model_and_batch(case)
            for step in range(steps):
                m.zero_grad(set_to_none=True)
                torch.manual_seed(100 + step)   # the loss draws sigma and the noise
                with recorded_calls() as calls:
                    try:
                        with torch.autocast("cuda", dtype=torch.float16, enabled=case["autocast"]):
                            loss = m.training_step(batch, step)
                        loss.backward()
                    except _lib.GeccoHipError as e:   # an entry point refused its arguments (nothing was launched): the route ends here
                        routes.append(calls + [f"raised: {e}"])
                        break
                torch.cuda.synchronize()
                routes.append(list(calls))
                if on_step is not None:
                    on_step(step, loss, m)
    finally:
        hip_ops.set_default_precision(prev)
        ag.WEIGHT_IMAGES.__init__()
    return routes
