from cutie_amd.inference.data.burst_test_dataset import BURSTTestDataset  # noqa: F401
