"""Reference datafactory/benchpress/dataloader.py: the names its drivers import, over datafactory/motion.py."""
from .. import motion
from ..motion import AlternatingDataset, custom_collate_fn  # noqa: F401  (reference names)
from .dataset import BenchpressT2SDataset


def loader_provider(args, period="train"):
    """(train_loader, test_loader): see datafactory.motion.loader_provider."""
    return motion.loader_provider(BenchpressT2SDataset, args, period)


def motion_groups(args, split="train"):
    """The three (N, C, L) training arrays of the dataset: see datafactory.motion.group_arrays."""
    return motion.group_arrays(BenchpressT2SDataset, args, split)
