"""cbfssm.utils: small helpers the run scripts and outputs of the reference import (cbfssm/utils/)."""
from .quaternions import Quaternion  # noqa: F401
