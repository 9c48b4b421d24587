"""Reference datafactory/benchpress/dataset.py: bench-press clips: 10 channels (feature_0..2, the barbell channels, are left out), length groups 36 / 72 / 144 with the
reference's thresholds (a clip shorter than 58 samples -> 36, 58..77 -> 72, 78 and longer -> 144), two stored embeddings.
A record is (text, x (10,T), Prefix_embedding, Summary_embedding, subject).
Everything but these constants is datafactory/motion.py's."""
from ..motion import MotionT2SDataset


class BenchpressT2SDataset(MotionT2SDataset):
    SKIP = ("feature_0", "feature_1", "feature_2")
    BASE, BOUNDS = 36, (58, 78)
    EMBEDDINGS = ("Prefix_embedding", "Summary_embedding")
