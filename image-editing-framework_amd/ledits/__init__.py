"""LEDITS++ method folder: masked multi-concept guidance on the edit-friendly DDPM noise space (`model/sd_utils.py`)."""
