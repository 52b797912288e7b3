"""Class maps between ModelNet40 and ScanObjectNN -- the label correspondence behind the reference README's
"Generalization of real vs synthetic" table, written from the two name lists (`training_data/shape_names_modelnet.txt`,
`shape_names_ext.txt`): a ModelNet40 class maps to the ScanObjectNN class of the same name, or through one of six aliases.
Everything else here is derived from that in code."""
from .pointnet2.evaluate_scenennobjects import SHAPE_NAMES as OBJECTDATASET_SHAPE_NAMES

# the 40 ModelNet40 categories in label order
MODELNET_SHAPE_NAMES = [
    "airplane", "bathtub", "bed", "bench", "bookshelf", "bottle", "bowl", "car", "chair", "cone",
    "cup", "curtain", "desk", "door", "dresser", "flower_pot", "glass_box", "guitar", "keyboard", "lamp",
    "laptop", "mantel", "monitor", "night_stand", "person", "piano", "plant", "radio", "range_hood", "sink",
    "sofa", "stairs", "stool", "table", "tent", "toilet", "tv_stand", "vase", "wardrobe", "xbox"]

# ModelNet40 names whose ScanObjectNN counterpart carries another name
ALIASES = {"bookshelf": "shelf", "dresser": "cabinet", "wardrobe": "cabinet", "monitor": "display", "bench": "chair",
           "stool": "chair"}
# ScanObjectNN's bag, bin, box and pillow have no ModelNet40 counterpart; "box" is NOT glass_box
_SAME_NAME = ("bed", "chair", "desk", "door", "sink", "sofa", "table", "toilet")


def _forward():
    target = dict({n: n for n in _SAME_NAME}, **ALIASES)
    return {i: OBJECTDATASET_SHAPE_NAMES.index(target[n]) for i, n in enumerate(MODELNET_SHAPE_NAMES) if n in target}


def _inverse(forward):
    inv = {}
    for m in sorted(forward):
        inv.setdefault(forward[m], []).append(m)
    return dict(sorted(inv.items()))


# ModelNet40 index -> ScanObjectNN index (many to one, fourteen entries)
MODELNET_TO_OBJECTDATASET = _forward()
# ScanObjectNN index -> the ModelNet40 indices that map to it (eleven keys)
OBJECTDATASET_TO_MODELNET = _inverse(MODELNET_TO_OBJECTDATASET)
# the eleven mapped ScanObjectNN classes numbered 0..10 in ascending order (read by no command line; for completeness)
OBJECTDATASET_TO_COMBINED = {o: i for i, o in enumerate(sorted(OBJECTDATASET_TO_MODELNET))}
