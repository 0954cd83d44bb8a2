"""DiffEdit method folder: inferred edit masks and a mask-preserving edit (`model/sd_utils.py`)."""
