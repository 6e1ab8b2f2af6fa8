"""Same import path as the reference's VLAAttacker/white_patch/UADA.py; implementation: roboticattack_amd.attack.uada."""
from roboticattack_amd.attack.uada import OpenVLAAttacker  # noqa: F401
from roboticattack_amd.constants import IGNORE_INDEX  # noqa: F401 (the reference module defines it: UADA.py:20)
