"""Rig absolute pose throughput and per-trial cost on one GPU, beside the single-camera absolute pose on the same machine
(DESIGN.md 13.9).

    python tools/rig_pose_bench.py [--queries 10000] [--points 1000] [--cameras 4] [--outliers 0.4] [--out FILE]

Reports, for Context.estimate_rig_absolute_poses and for Context.estimate_absolute_poses on a workload of the same shape:
the batch rate (end to end, kernel and device time), the trials run, the kernel time per trial over the batch, and the
kernel time of one query alone per trial of that query (the cost of a trial inside one wave).  Prints one JSON line."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

from pycolmap_amd import _capi, synth  # noqa: E402

W, H, F = 1600, 1200, 1200.0
MODELS = (0, 1, 2, 3)  # SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, RADIAL


def rig_queries(rng, num_queries, num_points, num_cameras, outlier_frac, noise_px=0.5):
    """num_queries rigs of num_cameras cameras (models cycling through MODELS, centres within 0.4 of the rig's origin),
    each seeing num_points random points in front of random cameras of the rig."""
    C, n = num_cameras, num_points
    models = np.array([MODELS[c % len(MODELS)] for c in range(C)], np.int32)
    prm = [np.asarray(synth._localisation_params(int(m), F, W, H), dtype=np.float64) for m in models]
    p2, p3 = np.zeros((num_queries * n, 2)), np.zeros((num_queries * n, 3))
    idx = np.zeros(num_queries * n, np.int32)
    rigs, qv, tv = np.zeros((num_queries * C, 7)), np.zeros((num_queries, 4)), np.zeros((num_queries, 3))
    for i in range(num_queries):
        Rr, qr = synth.random_rotation(rng)
        tr = -Rr @ rng.uniform(-5.0, 5.0, size=3)
        ci = rng.integers(0, C, size=n)
        u = rng.uniform(-0.45 * W / F, 0.45 * W / F, size=n)
        v = rng.uniform(-0.45 * H / F, 0.45 * H / F, size=n)
        d = rng.uniform(4.0, 12.0, size=n)
        Z = np.stack([u * d, v * d, d], axis=1)
        sl = slice(i * n, (i + 1) * n)
        for c in range(C):
            R, q = synth.random_rotation(rng)
            t = -R @ rng.uniform(-0.4, 0.4, size=3)
            rigs[i * C + c, :4], rigs[i * C + c, 4:] = q, t
            m = ci == c
            Y = (Z[m] - t) @ R               # R^T (Z - t)
            p3[sl][m] = (Y - tr) @ Rr
            p2[sl][m] = synth.img_from_cam(int(models[c]), prm[c], np.stack([u[m], v[m]], axis=1))
        p2[sl] += rng.normal(scale=noise_px, size=(n, 2))
        bad = rng.random(n) < outlier_frac
        p2[sl][bad] = np.stack([rng.uniform(0, W, int(bad.sum())), rng.uniform(0, H, int(bad.sum()))], 1)
        idx[sl] = ci
        qv[i], tv[i] = qr, tr
    return dict(offsets=np.arange(num_queries + 1, dtype=np.uint64) * n,
                camera_offsets=np.arange(num_queries + 1, dtype=np.uint64) * C, camera_models=np.tile(models, num_queries),
                camera_params=prm * num_queries, cams_from_rig=rigs, camera_idxs=idx, points2D=p2, points3D=p3, qvec=qv,
                tvec=tv)


def first_query(sc, rig):
    n = int(sc["offsets"][1])
    if not rig:
        return (sc["offsets"][:2], sc["camera_models"][:1], sc["camera_params"][:1], sc["points2D"][:n], sc["points3D"][:n])
    C = int(sc["camera_offsets"][1])
    return (sc["offsets"][:2], sc["camera_offsets"][:2], sc["camera_models"][:C], sc["camera_params"][:C],
            sc["cams_from_rig"][:C], sc["camera_idxs"][:n], sc["points2D"][:n], sc["points3D"][:n])


def measure(run, args, one, steps, truth_q):
    run(*one)  # warm-up
    single = [run(*one) for _ in range(5)]
    wall, kern, dev = [], [], []
    for _ in range(steps):
        t0 = time.perf_counter()
        r = run(*args)
        wall.append(time.perf_counter() - t0)
        kern.append(r["kernel_ms"])
        dev.append(r["device_ms"])
    ok = r["success"]
    nq = len(ok)
    dq = np.abs(np.abs((r["qvec"][ok] * truth_q[ok]).sum(1)) - 1.0)
    trials = int(r["num_trials"].sum())
    sk = float(np.median([s["kernel_ms"] for s in single]))
    return dict(queries_per_s=nq / float(np.median(wall)), wall_ms=1e3 * float(np.median(wall)),
                kernel_ms=float(np.median(kern)), device_ms=float(np.median(dev)), num_batches=r["num_batches"],
                success_rate=float(ok.mean()), max_quat_err=float(dq.max()) if dq.size else None, trials=trials,
                trials_per_query=trials / nq, batch_kernel_us_per_trial=1e3 * float(np.median(kern)) / max(trials, 1),
                single_query_kernel_ms=sk, single_query_trials=int(single[0]["num_trials"][0]),
                single_query_us_per_trial=1e3 * sk / max(int(single[0]["num_trials"][0]), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--cameras", type=int, default=4)
    ap.add_argument("--outliers", type=float, default=0.4)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = _capi.Context(0)
    sc = rig_queries(np.random.default_rng(0), a.queries, a.points, a.cameras, a.outliers)
    import rigpose_cases
    rig = measure(ctx.estimate_rig_absolute_poses, rigpose_cases.args(sc), first_query(sc, True), a.steps, sc["qvec"])
    ab = synth.localisation_scene(np.random.default_rng(0), a.queries, num_points=a.points, outlier_frac=a.outliers)
    abs_args = (ab["offsets"], ab["camera_models"], ab["camera_params"], ab["points2D"], ab["points3D"])
    single = measure(ctx.estimate_absolute_poses, abs_args, first_query(ab, False), a.steps, ab["qvec"])
    res = dict(workload=f"{a.queries} queries x {a.points} correspondences, {a.outliers:.0%} outliers; rig: {a.cameras} "
                        f"cameras (SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, RADIAL); absolute pose: SIMPLE_PINHOLE",
               rig_absolute_pose=rig, absolute_pose=single)
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
