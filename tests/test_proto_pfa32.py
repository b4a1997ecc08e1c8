"""tools/proto_pfa32.py -- the NumPy model of the 53 MS/s N-point plan (csrc/bds_acq_pfa32.h) -- holds: the index maps, the 25 x 25 rows
and the 32-point column stage as the lanes compute it all reproduce numpy.fft."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model():
    spec = importlib.util.spec_from_file_location("proto_pfa32", os.path.join(ROOT, "tools", "proto_pfa32.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_maps_rows_and_column_stage():
    m = _model()
    assert m.N == 1060000
    m.maps()
    m.rows()
    m.cols()
