from cutie_amd.inference.data.burst_video_reader import BURSTVideoReader  # noqa: F401
