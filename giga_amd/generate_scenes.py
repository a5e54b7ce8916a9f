"""`python -m giga_amd.generate_scenes`: packed scenes from a directory of object meshes, and the geometry data set they make.

    python -m giga_amd.generate_scenes --object-set data/urdfs/packed/train --raw data/set_raw --dataset data/set --num-scenes 1000

wraps `giga_amd.scenes.write_geo_dataset`: the kept objects of every scene (`mesh_pose_list/`), six depth images of the objects on
the table (`scenes/`, `setup.json`), occupancy labels (`occ/`), the fused grids under `--dataset` and a `grasps.csv` of placeholder
rows.  The result feeds `python -m giga_amd.train_geo` and `python -m giga_amd.eval_geometry` without `--ROI`; it holds no grasp
labels -- unless `--executor module:function` names a grasp executor (physics is not part of this package): then every scene gets
`--grasps-per-scene` labelled rows made from the fused cloud's normals (`giga_amd.candidates`).  A scene depends on `--seed` and its number alone (`--first-scene` continues a numbering); like the reference's scripts
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
    parser.add_argument("--executor", default=None, metavar="module:function",
                        help="grasp executor (scene, pos, quat, max_opening_width) -> (outcomes, widths): grasps.csv gets labelled rows")
    parser.add_argument("--grasps-per-scene", type=int, default=120)
    parser.add_argument("--num-rotations", type=int, default=6, help="yaw angles tried per grasp candidate")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    print(args)
    from .scenes import ObjectSet, write_geo_dataset
    objects = ObjectSet(args.object_set, args.global_scaling)
    execute = None
    if args.executor:
        from .candidates import resolve_executor
        execute = resolve_executor(args.executor)
    ids = write_geo_dataset(objects, args.raw, args.dataset, args.num_scenes, seed=args.seed, first_scene=args.first_scene,
                            batch=args.batch, n_views=args.views, num_point_per_file=args.num_point_per_file,
                            num_file=args.num_file, table_extent=args.table_extent, execute=execute,
                            grasps_per_scene=args.grasps_per_scene, num_rotations=args.num_rotations)
    if execute is not None:
        ids, unlabelled = ids
        print("%d scenes without an eligible cloud point got no grasp rows: %s" % (len(unlabelled), " ".join(unlabelled)))
    print("wrote %d scenes from %d objects" % (len(ids), len(objects)))


if __name__ == "__main__":
    main()
