from woft_amd.tracker import WOFTWindow, make_forward_compatible  # noqa: F401
from woft_amd.window import H_undo_crop  # noqa: F401
