"""`python -m giga_amd.generate_scenes`: packed scenes from a directory of object meshes, and the geometry data set they make.

    python -m giga_amd.generate_scenes --object-set data/urdfs/packed/train --raw data/set_raw --dataset data/set --num-scenes 1000

wraps `giga_amd.scenes.write_geo_dataset`: the kept objects of every scene (`mesh_pose_list/`), six depth images of the objects on
the table (`scenes/`, `setup.json`), occupancy labels (`occ/`), the fused grids under `--dataset` and a `grasps.csv` of placeholder
rows.  The result feeds `python -m giga_amd.train_geo` and `python -m giga_amd.eval_geometry` without `--ROI`; it holds no grasp
labels.  A scene depends on `--seed` and its number alone (`--first-scene` continues a numbering); like the reference's scripts
this one refuses to write into an existing data set."""
import argparse
from pathlib import Path


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m giga_amd.generate_scenes", description=__doc__.split("\n\n")[0])
    parser.add_argument("--object-set", type=Path, required=True, help="directory of one-link .urdf files (or of .obj files)")
    parser.add_argument("--raw", type=Path, required=True, help="raw root: mesh_pose_list/, scenes/, occ/, setup.json, grasps.csv")
    parser.add_argument("--dataset", type=Path, required=True, help="data set root: scenes/ (grids), point_clouds/")
    parser.add_argument("--num-scenes", type=int, default=100)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--first-scene", type=int, default=0)
    parser.add_argument("--batch", type=int, default=32, help="scenes per collision / render / fusion launch")
    parser.add_argument("--views", type=int, default=6, help="depth images per scene, on the reference's top-view circle")
    parser.add_argument("--num-point-per-file", type=int, default=2048)
    parser.add_argument("--num-file", type=int, default=4)
    parser.add_argument("--global-scaling", type=float, default=None, help="default: the reference's table, by directory name")
    parser.add_argument("--table-extent", type=float, default=0.6, help="side of the rendered table square")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    print(args)
    from .scenes import ObjectSet, write_geo_dataset
    objects = ObjectSet(args.object_set, args.global_scaling)
    ids = write_geo_dataset(objects, args.raw, args.dataset, args.num_scenes, seed=args.seed, first_scene=args.first_scene,
                            batch=args.batch, n_views=args.views, num_point_per_file=args.num_point_per_file,
                            num_file=args.num_file, table_extent=args.table_extent)
    print("wrote %d scenes from %d objects" % (len(ids), len(objects)))


if __name__ == "__main__":
    main()
