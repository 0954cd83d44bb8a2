"""Negative-prompt inversion with proximal guidance for the MasaCtrl folder (Han et al. publish proximal guidance on MasaCtrl): the
class of `p2p.inversion.npi`, which keeps the DDIM inversion and hands the edit the source embedding as its negative context.  The
MasaCtrl batch is [source, target] from `cat([x_T, x_T])`: row 0 follows the inversion back, row 1 is thresholded and pulled."""
from ...p2p.inversion.npi import NPI, negative_context  # noqa: F401
