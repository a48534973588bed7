"""What the command lines of the slide-map analyses share: finding the maps of a directory, reading one, refusing to run without a
device, writing a table.  Each piece written once; torch and PIL are imported inside the functions, as in _call.py."""
import csv
import glob
import os

import numpy as np


def require_device(what):
    """RuntimeError where there is no HIP device; `what` is the middle of the sentence: "the outlines are traced on the GPU\""""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device: %s, there is no host path" % what)


def map_paths(directory, suffix):
    """the files *<suffix> of `directory`, sorted; FileNotFoundError where there is none"""
    paths = sorted(glob.glob(os.path.join(directory, "*" + suffix)))
    if not paths:
        raise FileNotFoundError("no *%s under %s" % (suffix, directory))
    return paths


def slide_name(path, suffix):
    """<slide> of .../<slide><suffix>"""
    return os.path.basename(path)[:-len(suffix)]


def read_map(path):
    """the class map at `path`: uint8 [h,w], through composite.relabel; ValueError for an image of several channels"""
    from PIL import Image
    from .composite import relabel
    cm = relabel(np.ascontiguousarray(np.asarray(Image.open(path)), dtype=np.uint8))
    if cm.ndim != 2:
        raise ValueError("%s is not a single-channel class map" % path)
    return cm


def read_slide(path, suffix):
    """-> (slide_name, read_map)"""
    return slide_name(path, suffix), read_map(path)


def write_table(path, header, rows, delimiter=','):
    """the header and the rows as csv.writer writes them"""
    with open(path, 'w') as f:
        writer = csv.writer(f, delimiter=delimiter)
        writer.writerow(header)
        writer.writerows(rows)


def host(v):
    """a tensor or an array as a numpy array in host memory"""
    return np.asarray(v.cpu() if hasattr(v, "cpu") else v)
