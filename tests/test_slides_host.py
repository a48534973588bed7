"""What the command lines of the slide-map analyses share (glomeruli_segmentation_amd/_slides.py) and the binder of the modules'
own entry tables (_call.bound): the refusals with their exact texts, the slide name of a path, a map read back, a table written
and read back byte for byte.  No device."""
import ctypes

import numpy as np
import pytest

from glomeruli_segmentation_amd import _call, _lib, _slides
from glomeruli_segmentation_amd.instances import MAP_SUFFIX


def test_no_maps_and_no_device_are_refused_in_the_modules_words(tmp_path, monkeypatch):
    import torch
    with pytest.raises(FileNotFoundError) as e:
        _slides.map_paths(str(tmp_path), MAP_SUFFIX)
    assert str(e.value) == "no *_pred_classmap.png under %s" % tmp_path
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError) as e:
        _slides.require_device("the zones are computed on the GPU")
    assert str(e.value) == "no HIP device: the zones are computed on the GPU, there is no host path"
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    _slides.require_device("the zones are computed on the GPU")


def test_paths_names_and_maps(tmp_path):
    from PIL import Image
    cm = np.array([[0, 1, 2], [7, 8, 13]], dtype=np.uint8)           # the second row in Cityscapes ids: 0, 1, 4
    for name in ("b_slide", "a.slide"):
        Image.fromarray(cm).save(str(tmp_path / (name + MAP_SUFFIX)))
    Image.fromarray(cm).save(str(tmp_path / "a.slide_gt_classmap.png"))
    Image.fromarray(np.zeros((2, 3, 3), dtype=np.uint8)).save(str(tmp_path / "rgb.png"))
    paths = _slides.map_paths(str(tmp_path), MAP_SUFFIX)
    assert paths == [str(tmp_path / ("a.slide" + MAP_SUFFIX)), str(tmp_path / ("b_slide" + MAP_SUFFIX))]
    assert [_slides.slide_name(p, MAP_SUFFIX) for p in paths] == ["a.slide", "b_slide"]
    assert _slides.slide_name("/x/y/s1_outlines.geojson", "_outlines.geojson") == "s1"
    slide, got = _slides.read_slide(paths[0], MAP_SUFFIX)
    assert slide == "a.slide" and got.dtype == np.uint8 and got.tolist() == [[0, 1, 2], [0, 1, 4]]
    assert np.array_equal(_slides.read_map(paths[1]), got)
    with pytest.raises(ValueError) as e:
        _slides.read_map(str(tmp_path / "rgb.png"))
    assert str(e.value) == "%s is not a single-channel class map" % (tmp_path / "rgb.png")


def test_a_table_is_written_as_csv_writer_writes_it(tmp_path):
    header = ["slide", "id", "value", "note"]
    rows = [["s, 1", 1, 0.5, ""], ["s\t2", 2, 1e-07, 'say "x"'], ["s3", 3, float("nan"), "two\nlines"]]
    comma, tab = tmp_path / "t.csv", tmp_path / "t.tsv"
    _slides.write_table(str(comma), header, rows)
    _slides.write_table(str(tab), header, rows, delimiter='\t')
    assert comma.read_bytes() == (b'slide,id,value,note\r\n"s, 1",1,0.5,\r\ns\t2,2,1e-07,"say ""x"""\r\ns3,3,nan,"two\nlines"\r\n')
    assert tab.read_bytes() == (b'slide\tid\tvalue\tnote\r\ns, 1\t1\t0.5\t\r\n"s\t2"\t2\t1e-07\t"say ""x"""\r\ns3\t3\tnan\t"two\nlines"\r\n')
    _slides.write_table(str(comma), header, [])
    assert comma.read_bytes() == b'slide,id,value,note\r\n'


def test_host_takes_arrays_and_tensors():
    import torch
    a = np.arange(6, dtype=np.int32).reshape(2, 3)
    assert _slides.host(a) is a and np.array_equal(_slides.host(torch.from_numpy(a)), a) and _slides.host([1, 2]).tolist() == [1, 2]


def test_bound_is_the_library_with_the_table_set():
    from glomeruli_segmentation_amd import lesions, outlines, rasterize, zones
    lib = _lib.load()
    for module, table in ((outlines, outlines.OUTLINE_ENTRIES), (rasterize, rasterize.RASTER_ENTRIES), (zones, zones.ZONE_ENTRIES),
                          (lesions, lesions.LESION_ENTRIES)):
        assert _call.bound(table) is lib and module.load() is lib
        for name, (res, args) in table.items():
            fn = getattr(lib, name)
            assert fn.restype is res and list(fn.argtypes) == args
            assert not any(name in t for t in _lib.HEADERS.values())
    with pytest.raises(AttributeError):
        _call.bound({"gs_no_such_entry": (ctypes.c_int, [])})
