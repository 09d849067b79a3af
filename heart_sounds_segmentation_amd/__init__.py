"""heart_sounds_segmentation_amd -- MI355X-native FSST feature path (drop-in for the reference's
``hss.transforms.FSST`` + ``hss.moments``).  See DESIGN.md and INTEGRATION.md."""
from . import moments, transforms  # noqa: F401
from .transforms import FSST, Resample  # noqa: F401
from .consumer import segment_windowed  # noqa: F401
from .framing import cover_starts  # noqa: F401
from .sequence import (cyclic_transitions, decode_durations, decode_states, duration_counts_info, duration_nll,  # noqa: F401
                       duration_posteriors, duration_posteriors_info, durations_from_counts, durations_from_labels, edge_durations,
                       gaussian_durations, score_info, segmentation_scores, sequence_nll, state_posteriors, state_runs,
                       stitch_windows, transitions_from_labels, window_weights, SegmentationScores)

__all__ = ["FSST", "Resample", "moments", "transforms", "decode_states", "cyclic_transitions", "transitions_from_labels", "state_runs",
           "decode_durations", "edge_durations", "gaussian_durations", "durations_from_labels", "state_posteriors", "sequence_nll",
           "duration_posteriors", "duration_nll", "duration_posteriors_info", "durations_from_counts", "duration_counts_info",
           "segmentation_scores", "SegmentationScores", "score_info", "stitch_windows", "window_weights", "cover_starts",
           "segment_windowed"]

