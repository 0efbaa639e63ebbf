"""Supervised-learning path (mirror of keisei/sl/{dataset,trainer}.py): shard reader and SLTrainer, and two additions
the reference does not have: ``DeviceSLDataset`` (the positions packed in device memory) and ``prepare_sl_dataset``
(game records replayed straight into one; ``dataset_from_recorded_games`` does the same for the games a device
``GameLog`` recorded)."""

__all__ = ["DeviceSLDataset", "prepare_sl_dataset", "dataset_from_recorded_games"]


def __getattr__(name: str):
    # resolved on first use: ``python -m keisei_amd.sl.prepare`` must not find its module imported by its own package
    if name == "DeviceSLDataset":
        from keisei_amd.sl.device_dataset import DeviceSLDataset
        return DeviceSLDataset
    if name == "prepare_sl_dataset":
        from keisei_amd.sl.prepare import prepare_sl_dataset
        return prepare_sl_dataset
    if name == "dataset_from_recorded_games":
        from keisei_amd.sl.prepare import dataset_from_recorded_games
        return dataset_from_recorded_games
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
