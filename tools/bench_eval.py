"""Eval-mode timings of the detector (HIP events, after a warm-up of every shape; median and spread over --reps):

  detect : the eval-mode detector forward at c2 shapes (B = 16, N = 40000, C_in = 132) under no_grad, bf16 compute;
  val    : the c3 validation forward as the reference's lib/solver.py _feed runs it in phase "val" -- model.eval(), autograd
           enabled, forward + the losses, no backward;
  module : each detector module on its own (sa1..sa4, fp1, fp2, voting, vote_aggregation, proposal head), under no_grad.

    python tools/bench_eval.py [--reps 20] [--skip-val] [--out result.json]

Prints one JSON line.  Run it from two trees (this one and a checkout of another commit) to compare routes."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e))
    ts.sort()
    return {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1], "reps": reps}


def modules(model, pc, reps):
    """each module's forward on inputs captured from one detector forward"""
    bb, vote, prop = model.detection_backbone, model.voting_net, model.proposal_net
    xyz, feats = bb._break_up_pc(pc)
    out, ins = {}, {}
    with torch.no_grad():
        for i in (1, 2, 3, 4):
            sa = getattr(bb, "sa%d" % i)
            geo = sa.sample_and_query(xyz)
            ins["sa%d" % i] = (sa, xyz, feats, geo)
            xyz, feats, _ = sa(xyz, feats, geometry=geo)
        dd = bb({"point_clouds": pc})
        f1 = (dd["sa3_xyz"], dd["sa4_xyz"], dd["sa3_features"], dd["sa4_features"])
        ff = bb.fp1(*f1)
        f2 = (dd["sa2_xyz"], dd["sa3_xyz"], dd["sa2_features"], ff)
        vx, vf = vote(dd["fp2_xyz"], dd["fp2_features"])
        va = prop.vote_aggregation
        geo_v = va.sample_and_query(vx)
        _, agg, _ = va(vx, vf, geometry=geo_v)
        from bridgeqa_amd import pointnet2_utils as pu
        n1, n2 = pu.three_nn(f1[0], f1[1]), pu.three_nn(f2[0], f2[1])
    with torch.no_grad():
        for k, (sa, x, f, geo) in ins.items():
            out[k] = timed(lambda: sa(x, f, geometry=geo), reps)
        out["fp1"] = timed(lambda: bb.fp1(*f1, nn=n1), reps)
        out["fp2"] = timed(lambda: bb.fp2(*f2, nn=n2), reps)
        out["voting"] = timed(lambda: vote(dd["fp2_xyz"], dd["fp2_features"]), reps)
        out["vote_aggregation"] = timed(lambda: va(vx, vf, geometry=geo_v), reps)
        out["proposal_head"] = timed(lambda: prop._proposal_head(agg), reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--points", type=int, default=40000)
    ap.add_argument("--cin", type=int, default=132)
    ap.add_argument("--skip-val", action="store_true")
    ap.add_argument("--skip-modules", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench
    from bridgeqa_amd import fusion_ops
    dev = torch.device("cuda:0")
    fusion_ops.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    res = {"config": {k: v for k, v in vars(args).items() if k != "out"}}
    model = bench.build_model("c2", args.cin, 0).to(dev).eval()
    pc = bench.synth_batch(args.batch, args.points, args.cin, 42, dev)
    with torch.no_grad():
        res["detect"] = timed(lambda: model.detect({"point_clouds": pc}), args.reps)
    if not args.skip_modules:
        res["module"] = modules(model, pc, args.reps)
    del model
    if not args.skip_val:
        sys.argv = [sys.argv[0], "--workload", "c3"]
        bargs = bench.parse()
        bargs.batch, bargs.points, bargs.image = bargs.batch or 16, bargs.points or 40000, bargs.image or 512
        model = bench.build_model("c3", bargs.cin, bargs.image).to(dev).eval()
        batch = bench.make_batch(bargs, "c3", bargs.batch, 42, dev)
        batch["phase"] = "val"

        def val():
            dd = model(dict(batch))
            return bench.total_loss(dd)
        res["val"] = timed(val, args.reps)
        res["val"]["batch"] = bargs.batch
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
