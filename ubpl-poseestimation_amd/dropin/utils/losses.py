"""utils/losses.py on the HIP path (JointMSELoss, JointDistLoss, JointDistLoss_mt, JointDistLoss_mt2,
JointPseudoLoss, JointPseudoLoss2, JointPseudoLoss3, JointFeatureDistLoss, AvgCounter, AvgCounters)."""
from ubpl_amd.losses import (AvgCounter, AvgCounters, JointDistLoss, JointDistLoss_mt,  # noqa: F401
                             JointDistLoss_mt2, JointFeatureDistLoss, JointMSELoss, JointPseudoLoss,
                             JointPseudoLoss2, JointPseudoLoss3)
