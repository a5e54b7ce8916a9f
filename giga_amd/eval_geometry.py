"""`python -m giga_amd.eval_geometry`: the command line of the reference's scripts/eval_geometry_voxel.py on
`giga_amd.geometry.GeometryEvaluator`.

    python -m giga_amd.eval_geometry --model-path data/models/giga_geo.pt --type giga_geo --dataset data/set --dataset_raw data/set_raw --ROI

The flags of eval_geometry_voxel.py:165-175 with their defaults, plus `--batch` (scenes per encoder call), `--precision` (the
network's arithmetic), `--num-point-occ` (occupancy points per scene; 100000 as the reference's `create_test_loader`) and
`--n-points` (surface samples per mesh).  `--seed` keys every draw (`giga_amd.geometry`).  Results go to
`<logdir>/<time stamp>_eval_geo_dataset=...`: `%05d/results.json` per scene with `gt_mesh.ply` / `pred_mesh.ply` (the reference
writes `.glb`) and `mean_results.json`."""
import argparse
from datetime import datetime
from pathlib import Path


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m giga_amd.eval_geometry", description=__doc__.split("\n\n")[0])
    parser.add_argument("--model-path", type=str)
    parser.add_argument("--type", type=str)
    parser.add_argument("--dataset", type=Path, required=True)
    parser.add_argument("--dataset_raw", type=Path, required=True)
    parser.add_argument("--logdir", type=Path, default="data/eval_geo")
    parser.add_argument("--description", type=str, default="")
    parser.add_argument("--ROI", action="store_true", help="Use ROI occ point sampling")
    parser.add_argument("--th", type=float, default=0.5, help="level set threshold")
    parser.add_argument("--seed", type=int, default=42)
    parser.add_argument("--batch", type=int, default=8)
    parser.add_argument("--precision", choices=("fp32", "fp16", "fp16x3", "bf16", "fp16x3+fp16"), default="fp32")
    parser.add_argument("--num-point-occ", type=int, default=100000)
    parser.add_argument("--n-points", type=int, default=100000)
    return parser


def run_directory(args, now=None):
    """eval_geometry_voxel.py:29-37"""
    time_stamp = (now or datetime.now()).strftime("%y-%m-%d-%H-%M")
    description = "{}_eval_geo_dataset={},net={},th={},{}".format(
        time_stamp, args.dataset.name, args.type, args.th, args.description).strip(",")
    return Path(args.logdir) / description


def main(argv=None):
    args = build_parser().parse_args(argv)
    print(args)
    import torch

    from .geometry import GeometryEvaluator, VoxelOccGeoDataset, VoxelOccGeoROIDataset
    from .networks import load_network

    device = torch.device("cuda", torch.cuda.current_device())
    logdir = run_directory(args)
    logdir.mkdir(parents=True)
    cls = VoxelOccGeoROIDataset if args.ROI else VoxelOccGeoDataset
    dataset = cls(args.dataset, args.dataset_raw, num_point_occ=args.num_point_occ, seed=args.seed, device=device)
    net = load_network(args.model_path, device, model_type=args.type).eval().set_precision(args.precision)
    evaluator = GeometryEvaluator(net, threshold=args.th, n_points=args.n_points, batch=args.batch, seed=args.seed,
                                  model_path=args.model_path)
    results, mean = evaluator.evaluate(dataset, roi=args.ROI, logdir=logdir, export_meshes=True)
    for i, out in enumerate(results):
        if "empty" in out:
            print(f"{i} empty mesh!")
    print("Geometry prediction results:")
    for k, v in mean.items():
        if k != "model_path":
            print("%s: %.6f" % (k, v))


if __name__ == "__main__":
    main()
