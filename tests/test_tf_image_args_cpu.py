"""CPU: stabnet_tf_get_img refuses bad arguments with a status before it touches the device, and the Python table check names the
entry that is wrong."""
import numpy as np
import pytest


def test_bad_arguments_are_refused_without_a_gpu():
    from stabnet_amd import _lib
    L = _lib.lib()
    ok = [4096, 64, 4096, 1, 4096, 1, 2, 2, 1, 0, 0]            # pointers are never followed: every case fails a check before that
    for i, v in ((0, 0), (2, 0), (4, 0), (1, 2), (3, 0), (5, 0), (5, 65536), (6, 0), (7, 65537), (8, 0), (8, 33)):
        a = list(ok)
        a[i] = v
        assert L.stabnet_tf_get_img(*a) == -1, (i, v)
        assert b"tf_get_img" in L.stabnet_last_error()


def test_make_table_names_the_bad_entry():
    from stabnet_amd import _lib, tf_image
    good = (0, 4, 5, 15, 0, 0)
    t = tf_image.make_table([good, (60, 4, 5, 20, 1, 2)], 60 + 3 * 20 + 15, 2, 3)
    assert t.dtype == np.int64 and t.shape == (2, 6)
    for bad in ((1, 4, 5, 15, 0, 0), (0, 5, 5, 15, 0, 0), (0, 4, 5, 14, 0, 0), (-1, 4, 5, 15, 0, 0), (0, 0, 5, 15, 0, 0),
                (0, 4, 5, 15, 2, 0), (0, 4, 5, 15, 0, 3), (0, 4, 5, 15, -1, 0)):
        with pytest.raises(_lib.StabnetError) as e:
            tf_image.make_table([good, bad], 60, 2, 3)
        assert "entry 1" in str(e.value)
    with pytest.raises(_lib.StabnetError):
        tf_image.make_table([], 60, 2, 3)
