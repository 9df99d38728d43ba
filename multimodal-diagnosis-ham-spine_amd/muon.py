"""`from muon import MuonWithAuxAdam` of the reference's training script (scripts/train.py:262-307) resolves here when this
directory is on the path: the HIP implementation in hamspine.optim."""
from hamspine.optim import MuonWithAuxAdam

__all__ = ["MuonWithAuxAdam"]
