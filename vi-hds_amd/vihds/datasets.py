"""Plate-reader CSV loading, multi-file merge, scaling, device one-hots and the cross-validation split
(counterpart of the reference's vihds/datasets.py + data/procdata.py).  Host I/O only -- out of the hot path, kept
so that `run_xval.py <spec>.yaml` works on the reference's data files unchanged."""
import os
import warnings
from collections import OrderedDict

import numpy as np
import pandas as pd
import torch
from torch.utils.data import Dataset, Subset


def onehot(i, n):
    v = np.zeros((n))
    if i is not None:
        v[i] = 1
    return v


def depth(group_values):
    return len(set(g for g in group_values if g is not None))


def get_cassettes(devices, settings):
    """Concatenated one-hot blocks, one block per component group (reference datasets.py:26-45)."""
    rows = []
    for d in devices:
        name = settings.device_idx_to_device_name[d]
        rows.append(np.hstack([onehot(cm[name], depth(cm.values())) for cm in settings.component_maps.values()]))
    return np.array(rows).astype(np.float32)


def scale_data(X, settings):
    """Per-signal scaling to max 1 (or `normalize`), then per-series background subtraction (datasets.py:48-61)."""
    n_outputs = np.shape(X)[1]
    # (missing reads are NaN here: the maxima and the backgrounds are those of the reads that exist; a series without any
    # keeps its NaNs, which fill_unobserved replaces)
    complete = bool(np.isfinite(X).all())
    vmax, vmin = (np.max, np.min) if complete else (np.nanmax, np.nanmin)
    scales = settings.normalize if settings.normalize is not None else [
        vmax(X[:, i, :]).astype(np.float32) for i in range(n_outputs)]
    for i, scale in enumerate(scales):
        X[:, i, :] /= scale
        if settings.subtract_background:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)  # (nanmin of a series without a read)
                X[:, i, :] -= vmin(X[:, i, :], axis=1)[:, np.newaxis]
    return X, scales


def _parse_condition(text):
    """'C6=25000;C12=5' -> OrderedDict (reference data/procdata.py:15-28)."""
    d = OrderedDict()
    if "=" in text:
        for item in text.split(";"):
            k, v = item.split("=")
            d[k] = float(v)
    return d


def _signal_of(header):
    """'Raw Data (EYFP) 3 - 0 h 23 min' -> 'EYFP' (reference data/procdata.py:63-73)."""
    a = header.find("(")
    if a >= 0:
        b = header.find(")")
        if b >= 0:
            return header[a + 1: b]
    return header


def _readings(cells):
    """Reading cells -> float32; a blank cell or 'nan' is a missing read: NaN."""
    a = np.asarray(cells, dtype=object)
    flat = [np.nan if isinstance(v, str) and v.strip() == "" else float(v) for v in a.ravel()]
    return np.array(flat, dtype=np.float32).reshape(a.shape)


def load_csv(csv_file, settings):
    """One plate-reader file -> (devices [L], treatments [L,C], times [T], observations [L,4,T])
    (reference data/procdata.py:122-187): row 0 holds the time of every reading column; rows are kept when their
    device is listed in the spec and every condition not listed in the spec is zero.  A blank or 'nan' reading cell is an
    unobserved point: NaN in the returned observations (TimeSeriesDataset turns those into its `observed` mask)."""
    table = pd.read_csv(os.path.join(settings.data_dir, csv_file), sep=",", na_filter=False)
    timesall = table.iloc[0, 5:]
    body = table.iloc[1:, :]
    body = body.iloc[np.isin(body.iloc[:, 0], settings.devices), :]
    devices = np.array([settings.device_map[dev] for dev in body.iloc[:, 0]], dtype=int)
    treatments = [_parse_condition(c) for c in body.iloc[:, 4]]
    if len(treatments) == 0:
        return None
    keep, kept = [], []
    for i, tr in enumerate(treatments):
        if all(v == 0.0 for k, v in tr.items() if k not in settings.conditions):
            keep.append(i)
            kept.append([tr.get(c, 0.0) for c in settings.conditions])
    readings = body.iloc[keep, 5:]
    signals = np.array([_signal_of(str(h).split(".")[0]) for h in readings.columns.values])
    obs = np.array([[row.iloc[signals == s].values for s in settings.signals] for _, row in readings.iterrows()])
    times = timesall.iloc[signals == "OD"].values
    return (devices[keep] if len(keep) != len(devices) else devices, np.array(kept).astype(np.float32),
            times.astype(np.float32), _readings(obs))


def find_nearest(array, value):
    return (np.abs(np.asarray(array) - value)).argmin()


def fill_unobserved(times, observations, observed):
    """What the encoder sees of data with missing entries: observations [L,4,T] with every unobserved entry replaced, per row
    and signal, by the linear interpolant in time between its observed neighbours, by the nearest observed value before the
    first and after the last observed point, and by 0 for a signal without any observed point.  observed [L,4,T]: true where the
    read exists; whatever stands under a false entry (NaN, a saturated value) is not read.  Fully observed input is returned
    as it is."""
    observed = np.asarray(observed).astype(bool)
    if observed.all():
        return observations
    times = np.asarray(times, dtype=np.float64)
    out = np.array(observations, dtype=np.float32, copy=True)
    for row, flags in zip(out.reshape(-1, out.shape[-1]), observed.reshape(-1, observed.shape[-1])):
        if flags.all():
            continue
        at = np.flatnonzero(flags)
        if at.size == 0:
            row[:] = 0.0
        else:  # (np.interp holds the end values outside [times[at[0]], times[at[-1]]])
            row[~flags] = np.interp(times[~flags], times[at], row[at].astype(np.float64)).astype(np.float32)
    return out


def merge_union(times_list, observations_list, tolerance=0.0):
    """The files on the sorted union of their time points (spec: data.merge: union): times that differ by at most `tolerance`
    from the first time of a point are that point (0.0: exact equality).  Every file's rows hold their reads at the file's own
    points and NaN -- unobserved -- everywhere else: nothing is resampled, shifted or thrown away."""
    every = np.sort(np.unique(np.concatenate([np.asarray(t, dtype=np.float32) for t in times_list])))
    points = []
    for t in every:
        if not points or t - points[-1] > tolerance:
            points.append(t)
    points = np.array(points, dtype=np.float32)
    out = []
    for t, obs in zip(times_list, observations_list):
        t = np.asarray(t, dtype=np.float32)
        at = np.searchsorted(points, t, side="right") - 1  # (the point whose first time is the last one <= t)
        if len(set(at.tolist())) != len(at):
            raise ValueError("merge: union with merge_tolerance = %g puts two time points of one file into one point of the grid"
                             % tolerance)
        rows = np.full(obs.shape[:2] + (len(points),), np.nan, dtype=np.float32)
        rows[:, :, at] = obs
        out.append(rows)
    return points, np.concatenate(out)


def merge_observations(times_list, observations_list, merge=True, tolerance=0.0):
    """Resample every file onto the shortest file's time grid by nearest time (reference datasets.py:136-145;
    ragged inputs are kept as lists -- the reference's np.asarray of a ragged list fails on numpy >= 1.24).
    merge == "union": the sorted union of the files' time points instead (merge_union)."""
    if merge == "union":
        return merge_union(times_list, observations_list, tolerance)
    loc = int(np.argmin([len(t) for t in times_list]))
    chosen = times_list[loc]
    out = []
    for t, obs in zip(times_list, observations_list):
        locs = [find_nearest(t, ti) for ti in chosen]
        out.append(obs[:, :, locs])
    return chosen, np.concatenate(out)


class TimeSeriesDataset(Dataset):
    """reference datasets.py:64-124"""

    def __init__(self, data_settings, params):
        self.data_settings = data_settings
        self.params = params
        self.n_times = None
        self.n_species = None

    def _preprocess(self, devices, inputs, times, observations):
        self.devices = devices
        self.dev_1hot = torch.tensor(get_cassettes(devices, self.data_settings))
        self.inputs = torch.tensor(np.log(1.0 + inputs))
        self.times = torch.tensor(times)
        self.n_times = len(times)
        # missing entries (NaN: a blank cell, a point of the union grid another file has): the mask is kept as `observed` and
        # `observations` holds the filled array, so nothing non-finite reaches the encoder or the device
        flags = np.isfinite(observations)
        obs, self.scales = scale_data(observations, self.data_settings)
        self.observed = None
        if not flags.all():
            obs = fill_unobserved(times, obs, flags)
            self.observed = torch.tensor(flags.astype(np.float32))
        self.observations = torch.tensor(obs)
        self.n_species = np.shape(observations)[1]

    def init_single(self, f):
        self._preprocess(*load_csv(f, self.data_settings))

    def init_multiple_merge(self):
        loaded = [load_csv(f, self.data_settings) for f in self.data_settings.files]
        devices, inputs, times_list, obs_list = zip(*loaded)
        times, observations = merge_observations(list(times_list), list(obs_list), getattr(self.data_settings, "merge", True),
                                                 float(getattr(self.data_settings, "merge_tolerance", 0.0) or 0.0))
        self._preprocess(np.concatenate(devices), np.concatenate(inputs), times, observations)

    def __len__(self):
        return len(self.devices)

    def __getitem__(self, idx):
        if torch.is_tensor(idx):
            idx = idx.tolist()
        item = {"devices": self.devices[idx], "dev_1hot": self.dev_1hot[idx], "inputs": self.inputs[idx],
                "observations": self.observations[idx]}
        if getattr(self, "observed", None) is not None:  # (a dataset with missing entries only)
            item["observed"] = self.observed[idx]
        return item


class TimeSeriesDatasetPair(object):
    """reference datasets.py:148-170"""

    def __init__(self, train_dataset, test_dataset, data_settings):
        self.train, self.test = train_dataset, test_dataset
        self.n_train, self.n_test = len(train_dataset), len(test_dataset)
        self.depth = data_settings.device_depth
        self.n_conditions = len(data_settings.conditions)


def split_dataset(dataset, args, data_settings):
    """Seeded permutation split into `folds` chunks; chunk `split` is the validation set (datasets.py:199-222)."""
    np.random.seed(args.seed)
    if getattr(args, "heldout", None):
        raise NotImplementedError("TODO: implement heldout device")
    n = len(dataset)
    val_chunks = np.array_split(np.random.permutation(n), args.folds)
    val_ids = np.sort(val_chunks[args.split - 1])
    train_ids = np.setdiff1d(np.arange(n, dtype=int), val_ids)
    return TimeSeriesDatasetPair(Subset(dataset, train_ids), Subset(dataset, val_ids), data_settings)


def build_datasets(args, config):
    """reference datasets.py:173-224"""
    if not config.data.merge:
        raise NotImplementedError("Can't handle multiple datasets yet")  # as the reference's Encoder (encoders.py:363)
    dataset = TimeSeriesDataset(config.data, config.params)
    dataset.init_multiple_merge()
    return split_dataset(dataset, args, config.data)
