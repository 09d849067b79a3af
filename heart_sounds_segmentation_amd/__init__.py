"""heart_sounds_segmentation_amd -- MI355X-native FSST feature path (drop-in for the reference's
``hss.transforms.FSST`` + ``hss.moments``).  See DESIGN.md and INTEGRATION.md."""
from . import moments, transforms  # noqa: F401
from .transforms import FSST, Resample  # noqa: F401
from .consumer import cyclic_transitions, decode_states, state_runs, transitions_from_labels  # noqa: F401

__all__ = ["FSST", "Resample", "moments", "transforms", "decode_states", "cyclic_transitions", "transitions_from_labels", "state_runs"]
