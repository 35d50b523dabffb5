"""Side information of the data plane: item attributes, knowledge-graph features and visual feature vectors, narrowed together
with the rating frames and with each training fold.

What Elliot's `ItemAttributes`, `ChainedKG` and `VisualAttribute` loaders, their coordination and `DataSet`'s alignment with the
training fold produce, on this package's column frames.  One routine, `_settle`, serves both stages: it intersects the running (users, items) with what every
loader covers until nothing shrinks any more.

The contract that fixes the results is small.  The feature columns are `list({f for i in items for f in feature_map[i]})`, so their
order is the iteration order of CPython sets, and that depends on how the sets were built.  Three things are therefore kept exactly
and documented where they happen; everything else here is free:
  * the distinct users / items of a frame enter a set in order of first appearance; several frames are united test first;
  * every intersection has the running set on the LEFT and the loader's set on the right, a loader narrows its own sets with its own
    set on the left;
  * before a fold is aligned the loader's two sets are rebuilt from a list of their elements (what `copy.deepcopy` does to a set).
`feature_map` of `ItemAttributes` stays the unfiltered map of the file: TF-IDF counts its documents over it.  `ChainedKG` hands
out its REDUCED map instead (features of the selected properties that occur often enough, items that keep one), reduced again
every time the loader is narrowed.
"""
import os
from collections import Counter
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np

from .dataset import DataSet


def _get(ns, key, default=None):
    return ns.get(key, default) if isinstance(ns, dict) else getattr(ns, key, default)


def read_item_attributes(path):
    """{item id: list(set(feature ids))} of a TSV whose first field is the item and whose other fields are integer features."""
    with open(path) as fh:
        fields = (line.split("\t") for line in fh)
        return {int(f[0]): list(set(map(int, f[1:]))) for f in fields}


class ItemAttributes:
    """An attribute file and the users / items it currently stands for.  `get_mapped()` and `filter()` are the two calls Elliot's
    plug-ins and data sets expect of the `object` of a side-information namespace."""
    name = "ItemAttributes"

    def __init__(self, users, items, feature_map):
        self.users, self.items, self.feature_map = users, items, feature_map

    @classmethod
    def load(cls, users, items, spec, resolve):
        path = _get(spec, "attribute_file")
        if not path:
            raise Exception("side_information: the ItemAttributes loader needs `attribute_file`")
        feature_map = read_item_attributes(resolve(path))
        return cls(users, items & set(feature_map.keys()), feature_map)       # rated items left, the file's right

    def for_fold(self):
        """A loader of its own for one training fold: both sets rebuilt from lists, the attribute map shared (nothing writes it)."""
        return ItemAttributes(set(list(self.users)), set(list(self.items)), self.feature_map)

    def get_mapped(self):
        return self.users, self.items

    def filter(self, users, items):
        self.users, self.items = self.users & users, self.items & items       # the loader's own sets left

    def namespace(self):
        """What models read as `data.side_information.ItemAttributes`."""
        features = list({f for i in self.items for f in self.feature_map[i]})
        return SimpleNamespace(__name__=self.name, object=self, feature_map=self.feature_map, features=features,
                               nfeatures=len(features), private_features=dict(enumerate(features)),
                               public_features={f: p for p, f in enumerate(features)})


def read_feature_names(path):
    """{feature id: its chain of properties} of a `id \t <p1><p2>...<pn>` file, cut as the reference cuts it: the text behind the
    tab is split on '><', the first piece loses its first character and the last piece its last TWO ('>' and the newline -- a last
    line without a newline loses one character of the name)."""
    names = {}
    with open(path) as fh:
        for line in fh:
            fields = line.split("\t")
            chain = fields[1].split("><")
            chain[0] = chain[0][1:]
            chain[-1] = chain[-1][:-2]
            names[int(fields[0])] = chain
    return names


def read_properties(path):
    """The selected properties, one per line; lines that start with '#' are skipped."""
    with open(path) as fh:
        return [line.rstrip("\n") for line in fh if line[0] != "#"]


class ChainedKG:
    """Item features out of a knowledge graph (kahfm_style.py): a feature is a chain of properties that ends in an entity.  Of the
    file's map the loader keeps the features whose FIRST property is selected (`additive`) or is not selected (not `additive`) --
    all of them when no property is given -- and that occur more than `threshold` times among the current items; an item left
    without a feature leaves the loader.  The reduction runs at load and again whenever the loader is narrowed."""
    name = "ChainedKG"
    KEYS = ("map", "features", "properties")

    def __init__(self, users, items, map_, feature_names, properties, additive, threshold):
        self.users, self.items, self.map_ = users, items, map_
        self.feature_names, self.properties, self.additive, self.threshold = feature_names, properties, additive, threshold

    @classmethod
    def load(cls, users, items, spec, resolve):
        paths = {}
        for key in cls.KEYS:
            paths[key] = _get(spec, key)
            if not paths[key]:
                raise Exception(f"side_information: the ChainedKG loader needs `{key}` (its keys: map, features, properties; "
                                f"optional additive, threshold)")
        self = cls(users, items, read_item_attributes(resolve(paths["map"])), read_feature_names(resolve(paths["features"])),
                   read_properties(resolve(paths["properties"])), _get(spec, "additive", True), _get(spec, "threshold", 10))
        self._reduce()
        return self

    def _reduce(self):
        """reduce_attribute_map_property_selection, then the items that kept a feature (the loader's own set left)."""
        if not self.properties:
            acceptable = set(self.feature_names.keys())
        else:
            acceptable = {f for f, chain in self.feature_names.items() if (chain[0] in self.properties) == bool(self.additive)}
        narrowed = {k: v for k, v in self.map_.items() if k in self.items}
        count = Counter(f for fs in narrowed.values() for f in fs if f in acceptable)
        popular = {f for f, n in count.items() if n > self.threshold}
        reduced = {k: [f for f in v if f in popular] for k, v in narrowed.items()}
        self.map_ = {k: v for k, v in reduced.items() if len(v) > 0}
        self.items = self.items & set(self.map_.keys())

    def for_fold(self):
        """A loader of its own for one training fold: both sets rebuilt from lists, and a map of its own (`filter` rewrites it)."""
        return ChainedKG(set(list(self.users)), set(list(self.items)), {k: list(v) for k, v in self.map_.items()},
                         self.feature_names, self.properties, self.additive, self.threshold)

    def get_mapped(self):
        return self.users, self.items

    def filter(self, users, items):
        self.users, self.items = self.users & users, self.items & items       # the loader's own sets left
        self._reduce()

    def namespace(self):
        """What models read as `data.side_information.ChainedKG`; `feature_map` is the reduced map."""
        features = list({f for i in self.items for f in self.map_[i]})
        return SimpleNamespace(__name__=self.name, object=self, feature_map=self.map_, features=features,
                               nfeatures=len(features), private_features=dict(enumerate(features)),
                               public_features={f: p for p, f in enumerate(features)})


class VisualAttribute:
    """A folder of `<item id>.npy` files, one fp32 feature vector per item (visual_attribute.py).  The items are the rated items
    that have a file.  Their vectors are read ONCE, when the loader is made, by at most 16 threads, into one matrix that every
    fold shares; the row of an item is the file named by its PUBLIC id on the training path and on the evaluation path alike
    (DESIGN 3.28 has what the reference does instead).  `feature_matrix(items, device)` hands the rows out in the order asked
    for -- a data set's private-item order -- from one device copy that is uploaded at the first call."""
    name = "VisualAttributes"                                    # (the namespace's name in the reference, and VBPR's `loader` default)
    UNSUPPORTED = ("visual_pca_features", "visual_feat_map_features", "images_src_folder")
    MAX_READERS = 16

    def __init__(self, users, items, folder, item_mapping, store):
        self.users, self.items, self.folder, self.item_mapping, self.store = users, items, folder, item_mapping, store

    @classmethod
    def load(cls, users, items, spec, resolve):
        for key in cls.UNSUPPORTED:
            if _get(spec, key):
                raise Exception(f"side_information: `{key}` of the VisualAttribute loader is not supported by elliot_amd (it serves "
                                f"the image-based models; VBPR reads `visual_features` only)")
        folder = _get(spec, "visual_features")
        folder = resolve(folder) if folder else folder
        if not folder or not os.path.isdir(folder):
            raise Exception(f"side_information: the VisualAttribute loader needs `visual_features`, a folder of <item id>.npy files "
                            f"(got {folder!r}; dataloaders of elliot_amd: {sorted(LOADERS)})")
        stems = sorted(f[:-4] for f in os.listdir(folder) if f.endswith(".npy") and f[:-4].lstrip("-").isdigit())
        in_folder = set(int(s) for s in stems)
        item_mapping = {item: val for val, item in enumerate(in_folder)}          # the reference's field: position in the folder's set
        mine = items & in_folder                                                  # rated items left, the folder's right
        return cls(users, mine, folder, item_mapping, cls._read(folder, sorted(mine)))

    @classmethod
    def _read(cls, folder, ids):
        """{"ids": ascending public ids, "row": {id: row}, "matrix": fp32 [len(ids), D], "device": {}}; a file whose length is not
        the common one is refused with its name."""
        def one(item):
            return np.asarray(np.load(os.path.join(folder, f"{item}.npy")), dtype=np.float32).reshape(-1)
        with ThreadPoolExecutor(max_workers=max(1, min(cls.MAX_READERS, os.cpu_count() or 1))) as pool:
            vectors = list(pool.map(one, ids))
        lengths = Counter(len(v) for v in vectors)
        D = lengths.most_common(1)[0][0] if lengths else 0
        odd = [f"{item}.npy ({len(v)})" for item, v in zip(ids, vectors) if len(v) != D]
        if odd:
            raise Exception(f"side_information: visual feature files of another length than {D} in {folder}: {', '.join(odd[:8])}")
        matrix = np.stack(vectors) if vectors else np.zeros((0, 0), np.float32)
        return {"ids": list(ids), "row": {item: r for r, item in enumerate(ids)}, "matrix": matrix, "device": {}}

    def for_fold(self):
        """A loader of its own for one training fold: both sets rebuilt from lists; the matrix and its device copy are shared."""
        return VisualAttribute(set(list(self.users)), set(list(self.items)), self.folder, self.item_mapping, self.store)

    def get_mapped(self):
        return self.users, self.items

    def filter(self, users, items):
        self.users, self.items = self.users & users, self.items & items       # the loader's own sets left

    def feature_matrix(self, items, device=None):
        """fp32 [len(items), D]: row k is the vector of public item items[k].  device=None: a NumPy array; else a torch tensor on
        that device, gathered there from the one uploaded copy of the matrix."""
        missing = [i for i in items if i not in self.items]
        if missing:
            raise Exception(f"side_information: no visual features for items {missing[:8]} (not among the loader's items)")
        rows = np.fromiter((self.store["row"][i] for i in items), dtype=np.int64, count=len(items))
        if device is None:
            return self.store["matrix"][rows]
        import torch
        key = str(device)
        if key not in self.store["device"]:
            self.store["device"][key] = torch.from_numpy(self.store["matrix"]).to(device)
        whole = self.store["device"][key]
        if len(rows) == whole.shape[0] and np.array_equal(rows, np.arange(len(rows))):
            return whole
        return whole.index_select(0, torch.from_numpy(rows).to(device)).contiguous()

    def namespace(self):
        """What models read as `data.side_information.VisualAttributes`: the reference's field names plus `feature_matrix`."""
        return SimpleNamespace(__name__=self.name, object=self, visual_feature_folder_path=self.folder, item_mapping=self.item_mapping,
                               visual_features_shape=int(self.store["matrix"].shape[1]), feature_matrix=self.feature_matrix)


LOADERS = {"ItemAttributes": ItemAttributes, "ChainedKG": ChainedKG, "VisualAttribute": VisualAttribute}


def _settle(users, items, loaders):
    """Narrow (users, items) and every loader to what all of them cover.  A round intersects the running sets with each loader's
    in turn; when no set involved changed size the round's result stands, otherwise the loaders narrow themselves and another round
    follows.  Returns the settled (users, items)."""
    while True:
        settled = True
        for theirs_u, theirs_i in [ld.get_mapped() for ld in loaders]:
            both_u, both_i = users & theirs_u, items & theirs_i
            settled &= len(users) == len(theirs_u) == len(both_u) and len(items) == len(theirs_i) == len(both_i)
            users, items = both_u, both_i
        if settled:
            return users, items
        for ld in loaders:
            ld.filter(users, items)


def _namespaces(loaders):
    out = SimpleNamespace()
    for ld in loaders:
        setattr(out, ld.name, ld.namespace())
    return out


def _distinct(column):
    """The distinct values of a frame column as a set filled in order of first appearance."""
    return set(DataSet._first_appearance(np.asarray(column)).tolist())


def _map_frames(frames, fn):
    """`fn` over every frame of one frame, a (train, test) tuple list, or a ([(train, val), ...], test) tuple list."""
    if isinstance(frames, dict):
        return fn(frames)
    return [([(fn(tr), fn(va)) for tr, va in train] if isinstance(train, list) else fn(train), fn(test)) for train, test in frames]


def coordinate(frames, sides, logger=None, resolve=lambda p: p):
    """Load the configured side information and cut frames and loaders down to each other.  `frames`: one frame (strategy: dataset,
    before prefiltering and splitting) or the loader's tuple list (strategy: fixed); `sides`: data_config.side_information.
    Users and items start as those of the frames -- of the first test fold, then its train (and validation) frame when there are
    several.  Returns (frames with only the surviving rows, namespace of side information)."""
    if isinstance(frames, dict):
        seen = [frames]
    else:
        train, test = frames[0]
        seen = [test] + (list(train[0]) if isinstance(train, list) else [train])
    users, items = set(), set()
    for fr in seen:
        users, items = users | _distinct(fr["userId"]), items | _distinct(fr["itemId"])
    loaders = []
    for spec in sides or []:
        kind = _get(spec, "dataloader")
        if kind not in LOADERS:
            raise Exception(f"side_information: dataloader {kind!r} is not provided by elliot_amd (supported: {sorted(LOADERS)})")
        loaders.append(LOADERS[kind].load(users, items, spec, resolve))
    users, items = _settle(users, items, loaders)
    keep_u, keep_i = np.array(list(users)), np.array(list(items))

    def surviving(fr):
        rows = np.isin(fr["userId"], keep_u) & np.isin(fr["itemId"], keep_i)
        return {c: v[rows] for c, v in fr.items()}
    return _map_frames(frames, surviving), _namespaces(loaders)


def align_with_training(train_users, train_items_dict_order, side_information):
    """The side information of ONE training fold: every loader is copied (`for_fold`), settled against the fold's users and items
    and asked for a fresh namespace; `side_information` itself stays as it is for the next fold.  train_users: the fold's users in
    first-appearance order (the keys of train_dict); train_items_dict_order: its items user after user in train_dict order (repeats
    allowed) -- they fill a set in that order, and the fold works on a copy of that set."""
    loaders = [ns.object.for_fold() for ns in vars(side_information).values()]
    _settle(set(train_users), set({i for i in train_items_dict_order}), loaders)
    return _namespaces(loaders)
