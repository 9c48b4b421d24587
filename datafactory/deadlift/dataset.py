"""Reference datafactory/deadlift/dataset.py: deadlift clips: 7 channels, clips shorter than 10 samples dropped, length groups 48 / 96 / 192 with the reference's
thresholds (a clip shorter than 81 samples -> 48, 81..98 -> 96, 99 and longer -> 192), one stored embedding.
A record is (text, x (7,T), embedding, subject).
Everything but these constants is datafactory/motion.py's."""
from ..motion import MotionT2SDataset


class DeadliftT2SDataset(MotionT2SDataset):
    MIN_T = 10
    BASE, BOUNDS = 48, (81, 99)
    EMBEDDINGS = ("embedding",)
