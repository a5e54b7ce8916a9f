"""`python -m giga_amd.train`: the command line of the reference's scripts/train_giga.py on `giga_amd.trainer.Trainer`.

    python -m giga_amd.train --dataset data/set --dataset_raw data/set_raw --net giga --augment --precision bf16

The flags of train_giga.py:250-262 with their defaults, plus `--precision` (arithmetic of the training step), `--seed` (split,
epoch orders and draws) and `--resume` (continue the run in `--savedir`, which it requires).  `--silence` is accepted and changes
nothing: it hides the reference's progress bar, and there is none here.  The whole set is read once into device memory
(`ResidentTrainingSet`); the train batches are shuffled, both iterators drop the last short batch, as the reference's loaders do.
Under `torchrun` every rank takes its share of each epoch's order and the flat gradient is averaged over the ranks."""
import argparse
import os
from datetime import datetime
from pathlib import Path


def build_parser(prog="python -m giga_amd.train", description=None, net="giga", nets=None):
    """the flags; `net` is the default of `--net` and `nets`, when given, its choices (`python -m giga_amd.train_geo` shares them)"""
    parser = argparse.ArgumentParser(prog=prog, description=description or __doc__.split("\n\n")[0])
    parser.add_argument("--net", default=net, choices=nets)
    parser.add_argument("--dataset", type=Path, required=True)
    parser.add_argument("--dataset_raw", type=Path, required=True)
    parser.add_argument("--logdir", type=Path, default="data/runs")
    parser.add_argument("--description", type=str, default="")
    parser.add_argument("--savedir", type=str, default="")
    parser.add_argument("--epochs", type=int, default=10)
    parser.add_argument("--batch-size", type=int, default=32)
    parser.add_argument("--lr", type=float, default=2e-4)
    parser.add_argument("--val-split", type=float, default=0.1)
    parser.add_argument("--augment", action="store_true")
    parser.add_argument("--silence", action="store_true")
    parser.add_argument("--load-path", type=str, default="")
    parser.add_argument("--precision", choices=("fp32", "bf16", "bf16_convs"), default="fp32")
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--resume", action="store_true")
    return parser


def run_directory(args, now=None):
    """train_giga.py:25-38: `--savedir`, or `--logdir` / a name made of the time stamp and the settings"""
    if args.savedir != "":
        return Path(args.savedir)
    time_stamp = (now or datetime.now()).strftime("%y-%m-%d-%H-%M")
    description = "{}_dataset={},augment={},net={},batch_size={},lr={:.0e},{}".format(
        time_stamp, args.dataset.name, args.augment, args.net, args.batch_size, args.lr, args.description).strip(",")
    return Path(args.logdir) / description


def parse_args(argv=None, parser=None):
    parser = parser or build_parser()
    args = parser.parse_args(argv)
    if args.resume and args.savedir == "":                   # (without it the directory's name carries the time of THIS start)
        parser.error("--resume continues the run in --savedir: name that directory")
    return args


def main(argv=None, parser=None, trainer_class=None):
    """parse, read the set, build the network and run the epochs; `parser` and `trainer_class` (default: this module's flags and
    `Trainer`) are what `python -m giga_amd.train_geo` replaces"""
    args = parse_args(argv, parser)
    import torch
    import torch.distributed as dist

    from .dataset import GraspOccDataset
    from .networks import get_network, load_network
    from .resident import ResidentBatches, ResidentTrainingSet
    from .trainer import Trainer, train_val_split

    rank, world, group = 0, 1, None
    if "RANK" in os.environ and "WORLD_SIZE" in os.environ:                     # started by torchrun
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", 0)))
        dist.init_process_group("nccl")
        rank, world, group = dist.get_rank(), dist.get_world_size(), dist.group.WORLD
    if rank == 0:
        print(args)
    device = torch.device("cuda", torch.cuda.current_device())
    rset = ResidentTrainingSet(GraspOccDataset(args.dataset, args.dataset_raw, augment=args.augment), device=device)
    train_idx, val_idx = train_val_split(len(rset), args.val_split, args.seed)
    train = ResidentBatches(rset, args.batch_size, shuffle=True, seed=args.seed, drop_last=True, indices=train_idx, rank=rank, world=world)
    val = ResidentBatches(rset, args.batch_size, shuffle=False, seed=args.seed, drop_last=True, indices=val_idx, rank=rank, world=world)
    net = get_network(args.net).to(device) if args.load_path == "" else load_network(args.load_path, device, args.net)
    logdir = [run_directory(args) if rank == 0 else None]
    if group is not None:                                    # one name for all ranks: rank 0's (the time stamp is its clock's)
        dist.broadcast_object_list(logdir, src=0)
    # --silence hides the reference's progress bar and nothing else; there is no bar here, so the flag changes nothing.  The ranks'
    # networks differ at this point (torch's initialisation): the Trainer broadcasts rank 0's
    trainer = (trainer_class or Trainer)(net, train, val, lr=args.lr, net_name=args.net, logdir=logdir[0], precision=args.precision,
                                         group=group, resume=args.resume)
    trainer.run(args.epochs)
    if group is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
