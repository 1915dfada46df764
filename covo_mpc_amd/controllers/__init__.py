"""quadjax/controllers/__init__.py:1-7 re-exports."""
from .base import BaseController  # noqa: F401
from .random import RandomController  # noqa: F401
from .pid import PIDController, PIDParams  # noqa: F401
from .mppi import MPPIController, MPPIParams  # noqa: F401
from .covo import CoVOController, CoVOParams  # noqa: F401
from .batched import BatchedCMAController, BatchedCoVOController, BatchedDialController, BatchedILQRController, BatchedMPPIController  # noqa: F401
from .ilqr import ILQRBoxController, ILQRController, ILQRParams  # noqa: F401
from .dial import DialController  # noqa: F401
from .cma import CMAController, CMAParams  # noqa: F401
from .estimator import StateEstimator  # noqa: F401
from .observer import ForceObserver  # noqa: F401
