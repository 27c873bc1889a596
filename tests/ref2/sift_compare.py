"""Deviation budget of the SIFT reference.

Runs a fixed set of small seeded images through
  * the CPU reference tests/sift_ref/sift_ref.cc (float32, bit-identical to sift.hip), the candidate, and
  * the independent float64 restatement tests/ref2/sift_ref2.py, the judge, with the project's exp / atan2
    approximations restated (approx=True) and with libm in their place (approx=False),
pairs the features of the two sides and reports (with ref2 following the project's rule of deviation S10; what that
rule costs is recorded beside it, under "s10", as the features left without a partner when ref2 follows Lowe's), per image and mode: the feature counts, the share of features on each
side without a partner, the distance d of the partners, and the distance of their descriptors.

A partner is the nearest feature of the other side under

    d = pixel distance / min(sigma) + |ln(sigma ratio)| + |angle difference wrapped to (-pi, pi]|

and a pair counts if d < 0.05.  Runs with upright=True carry no angle term: they isolate the scale space, detection and
refinement from the orientation histogram.

  python tests/ref2/sift_compare.py [--out tests/ref2/sift_deviation_budget.json]

`measure` takes any candidate, so the GPU suite holds Context.sift_extract to the same judge with the same limits.
"""
from __future__ import annotations

import argparse
import functools
import json
import math
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "tests"))

import sift_images as si  # noqa: E402
from ref2 import sift_ref2  # noqa: E402

PAIR_LIMIT = 0.05

IMAGES = {
    "textured": lambda: si.textured(1, 96, 128),
    "noise": lambda: si.noise(2, 61, 77),
    "rendered": lambda: si.render(si.plane_texture(3, 512), si.similarity(12.0, 0.9, 5.0, -3.0, 130, 100), 120, 160),
    "blobs": lambda: si.blobs(128, 160, [(40.3, 50.7, 3.0), (100.2, 80.4, 5.0), (60.0, 30.0, 2.0)]),
}
ORIENTED = ("textured", "noise", "rendered")     # the orientation of an isotropic blob is not defined


def cases():
    """[(tag, image name, options)]: every image at first_octave -1 and 0, oriented and upright; then octave_resolution
    2 and 4 and first_octave 1 on the textured and the rendered image."""
    out = []
    for name in IMAGES:
        for fo in (-1, 0):
            if name in ORIENTED:
                out.append((f"{name}/o{fo}", name, dict(first_octave=fo)))
            out.append((f"{name}/o{fo}/upright", name, dict(first_octave=fo, upright=True)))
    for name in ("textured", "rendered"):
        out.append((f"{name}/o0/S2", name, dict(first_octave=0, octave_resolution=2)))
        out.append((f"{name}/o0/S4", name, dict(first_octave=0, octave_resolution=4)))
        out.append((f"{name}/o1", name, dict(first_octave=1)))
    return out


# the sample the CPU and GPU suites run (every image, every mode of the options, about a second each)
FAST = ("textured/o0", "noise/o-1", "rendered/o0", "blobs/o0/upright", "textured/o0/upright", "textured/o0/S2",
        "rendered/o0/S4", "rendered/o1")


def partners(kp_a: np.ndarray, kp_b: np.ndarray, with_angle: bool):
    """For every feature of a: (index of its nearest feature of b under d, that d); (-1, inf) when b is empty."""
    if len(kp_a) == 0 or len(kp_b) == 0:
        return np.full(len(kp_a), -1), np.full(len(kp_a), np.inf)
    a, b = np.asarray(kp_a, np.float64)[:, None, :], np.asarray(kp_b, np.float64)[None, :, :]
    d = np.hypot(a[..., 0] - b[..., 0], a[..., 1] - b[..., 1]) / np.minimum(a[..., 2], b[..., 2])
    d = d + np.abs(np.log(a[..., 2] / b[..., 2]))
    if with_angle:
        diff = a[..., 3] - b[..., 3]
        d = d + np.abs(diff - 2.0 * math.pi * np.ceil((diff - math.pi) / (2.0 * math.pi)))    # (-pi, pi]
    j = np.argmin(d, axis=1)
    return j, d[np.arange(len(j)), j]


def measure(candidate, judge, with_angle: bool) -> dict:
    """The entry of one image and mode: `candidate` and `judge` are (keypoints, descriptor bytes)."""
    (ck, cd), (jk, jd) = candidate, judge
    j, dc = partners(ck, jk, with_angle)
    _, dj = partners(jk, ck, with_angle)
    paired = dc < PAIR_LIMIT
    a = np.asarray(cd, np.float64)[paired]
    b = np.asarray(jd, np.float64)[j[paired]]
    rel = np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1) if len(a) else np.zeros(0)
    return dict(
        features=[int(len(ck)), int(len(jk))],
        unpaired=[int((~paired).sum()), int((dj >= PAIR_LIMIT).sum())],
        unpaired_share=[float((~paired).mean()) if len(ck) else 0.0,
                        float((dj >= PAIR_LIMIT).mean()) if len(jk) else 0.0],
        d_median=float(np.median(dc[paired])) if paired.any() else 0.0,
        d_max=float(dc[paired].max()) if paired.any() else 0.0,
        byte_diff_max=int(np.abs(a - b).max()) if len(a) else 0,
        byte_diff_share=float((a != b).mean()) if len(a) else 0.0,
        rel_l2_median=float(np.median(rel)) if len(rel) else 0.0,
        rel_l2_max=float(rel.max()) if len(rel) else 0.0,
    )


@functools.lru_cache(maxsize=None)
def image(name: str) -> np.ndarray:
    img = IMAGES[name]()
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _judge(name: str, opts: tuple, approx: bool, move_after_last_solve: bool):
    return sift_ref2.extract(image(name), approx=approx, move_after_last_solve=move_after_last_solve, **dict(opts))


def judge_of(name: str, opts: dict, approx: bool, move_after_last_solve: bool = True):
    """ref2 on one case; computed once per process and shared (the CPU and the GPU suite ask for the same cases)"""
    return _judge(name, tuple(sorted(opts.items())), approx, move_after_last_solve)


def s10_entry(candidate, name: str, opts: dict) -> dict:
    """What deviation S10 costs on one case: the candidate against ref2 with Lowe's rule in place of the project's
    (approx=True, so that nothing else differs)."""
    e = measure(candidate, judge_of(name, opts, True, move_after_last_solve=False),
                with_angle=not opts.get("upright", False))
    return dict(features=e["features"], unpaired=e["unpaired"])


def evaluate(tags=None, verbose: bool = True) -> dict:
    import sift_ref_lib as ref
    entries, s10 = {}, {}
    for tag, name, opts in cases():
        if tags is not None and tag not in tags:
            continue
        cand = ref.extract(image(name), **opts)
        s10[tag] = s10_entry(cand, name, opts)
        for approx in (True, False):
            e = measure(cand, judge_of(name, opts, approx), with_angle=not opts.get("upright", False))
            entries[f"{tag}/{'approx' if approx else 'libm'}"] = e
            if verbose:
                print(f"{tag:24s} {'approx' if approx else 'libm':6s} features {e['features']} "
                      f"unpaired {e['unpaired']} "
                      f"d max {e['d_max']:.2e} bytes max {e['byte_diff_max']} share {e['byte_diff_share']:.4f} "
                      f"rel L2 max {e['rel_l2_max']:.4f}")
    if verbose:
        print("S10 (Lowe's rule after the fifth solve): without a partner",
              [sum(e["unpaired"][i] for e in s10.values()) for i in (0, 1)], "of",
              [sum(e["features"][i] for e in s10.values()) for i in (0, 1)])
    return dict(pair_limit=PAIR_LIMIT, entries=entries, limits=limits_of(entries), s10=s10)


def limits_of(entries: dict) -> dict:
    """The recorded maxima per mode over the entries the conditions cover (oriented runs of the oriented images, upright
    runs of every image): what the tests double (continuous quantities) or take as is (byte steps)."""
    out = {}
    for mode in ("approx", "libm"):
        es = [e for t, e in entries.items() if t.endswith("/" + mode)]
        out[mode] = dict(d_max=max(e["d_max"] for e in es), byte_diff_max=max(e["byte_diff_max"] for e in es),
                         byte_diff_share=max(e["byte_diff_share"] for e in es),
                         rel_l2_max=max(e["rel_l2_max"] for e in es),
                         features=[sum(e["features"][i] for e in es) for i in (0, 1)],
                         unpaired=[sum(e["unpaired"][i] for e in es) for i in (0, 1)])
    return out


CASES = {tag: (name, opts) for tag, name, opts in cases()}


def budget() -> dict:
    return json.loads(Path(__file__).with_name("sift_deviation_budget.json").read_text())


def check_against_budget(tag: str, candidate) -> None:
    """Hold one candidate's (keypoints, descriptors) on one case to ref2 within the committed limits (DESIGN.md section
    10.10): twice the recorded maximum for the continuous quantities, the recorded integer for byte steps.  Prints each
    figure before it asserts."""
    name, opts = CASES[tag]
    upright = bool(opts.get("upright", False))
    limits = budget()["limits"]
    for mode, approx in (("approx", True), ("libm", False)):
        e = measure(candidate, judge_of(name, opts, approx), with_angle=not upright)
        lim = limits[mode]
        print(tag, mode, json.dumps(e))
        assert min(e["features"]) > 0, (tag, mode, e["features"])
        if approx or upright:       # every feature on either side has a partner
            assert e["unpaired"] == [0, 0], (tag, mode, e["unpaired"])
        else:                       # libm in place of the approximations: at most 2 % without one
            assert max(e["unpaired_share"]) <= 0.02, (tag, mode, e["unpaired_share"])
        assert e["byte_diff_max"] <= lim["byte_diff_max"], (tag, mode, e["byte_diff_max"], lim["byte_diff_max"])
        for key in ("d_max", "byte_diff_share", "rel_l2_max"):
            assert e[key] <= 2.0 * lim[key], (tag, mode, key, e[key], lim[key])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(Path(__file__).with_name("sift_deviation_budget.json")))
    args = ap.parse_args()
    Path(args.out).write_text(json.dumps(evaluate(), indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
