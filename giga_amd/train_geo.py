"""`python -m giga_amd.train_geo`: the command line of the reference's scripts/train_giga_geo.py on `giga_amd.trainer.GeoTrainer`.

    python -m giga_amd.train_geo --dataset data/set --dataset_raw data/set_raw --precision bf16

The flags of train_giga_geo.py:218-233 with their defaults (`--net` is `giga_geo`; any other net is an error: `giga_amd.train`
runs those), plus `--precision`, `--seed` and `--resume` as `giga_amd.train` has them.  The set is the one `giga_amd.train` reads,
the grasp rows of `DatasetVoxelOccFile`; the occupancy-only model uses each row's grid and occupancy points and ignores its grasp.
`--augment` is honoured here.  The reference's script accepts the flag and then drops it (it builds
`DatasetVoxelOccFile(root, root_raw)`, train_giga_geo.py:124, so its sets are never augmented); the default, no augmentation, is
therefore the reference's behaviour.  The result is `vgn_giga_geo_<iteration>.pt`, which `python -m giga_amd.eval_geometry --type
giga_geo` scores."""
from . import train

NET = "giga_geo"


def build_parser():
    return train.build_parser(prog="python -m giga_amd.train_geo", description=__doc__.split("\n\n")[0], net=NET, nets=(NET,))


def parse_args(argv=None):
    return train.parse_args(argv, build_parser())


def main(argv=None):
    from .trainer import GeoTrainer
    train.main(argv, parser=build_parser(), trainer_class=GeoTrainer)


if __name__ == "__main__":
    main()
