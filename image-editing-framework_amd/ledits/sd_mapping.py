"""`sd_version -> model location`; same table as the P2P folder."""
from ..p2p.sd_mapping import sd_maps  # noqa: F401
