from cutie_amd.inference.utils.burst_utils import BURSTResultHandler  # noqa: F401
