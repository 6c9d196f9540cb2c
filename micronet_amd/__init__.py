from . import pruning  # noqa: F401
from .pruning import bn_threshold, compact, gc_prune_cfg, regular_prune  # noqa: F401
