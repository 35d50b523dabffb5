"""Side information of the data plane: item attributes, narrowed together with the rating frames and with each training fold.

What Elliot's `ItemAttributes` loader, its loader coordination and `DataSet`'s alignment with the training fold produce, on this
package's column frames.  One routine, `_settle`, serves both stages: it intersects the running (users, items) with what every
loader covers until nothing shrinks any more.

The contract that fixes the results is small.  The feature columns are `list({f for i in items for f in feature_map[i]})`, so their
order is the iteration order of CPython sets, and that depends on how the sets were built.  Three things are therefore kept exactly
and documented where they happen; everything else here is free:
  * the distinct users / items of a frame enter a set in order of first appearance; several frames are united test first;
  * every intersection has the running set on the LEFT and the loader's set on the right, a loader narrows its own sets with its own
    set on the left;
  * before a fold is aligned the loader's two sets are rebuilt from a list of their elements (what `copy.deepcopy` does to a set).
`feature_map` stays the unfiltered map of the file: TF-IDF counts its documents over it.
"""
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


LOADERS = {"ItemAttributes": ItemAttributes}


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
