"""jds_pjpeg_parse against tests/golden/pjpeg_parse_pins.json (no GPU): the return code, the
message and the struct bytes on small pure-Python progressive files (the scan scripts over two
geometries, the 64-scan gray file, a baseline file), on every byte of their headers and of the
marker segments between their scans set to each of sixteen values, and on their truncations;
and the named files with two defects, whose report depends on the order of the checks.  The
fixture was recorded from the build before the progressive walk was put on the baseline walk's
pieces (tests/golden/make_parse_pins.py --pjpeg), never from the code under test: the parser
must answer as it did."""
import importlib.util
import json
import os

import pytest

from conftest import ROOT

_spec = importlib.util.spec_from_file_location(
    'make_parse_pins', os.path.join(ROOT, 'tests', 'golden', 'make_parse_pins.py'))
mp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mp)

PINS = json.load(open(mp.PJPEG_PINS))
SOURCES = sorted(PINS['sources'])
PARSER = 'pjpeg'


@pytest.fixture(scope='module')
def lib():
    from jds import _abi, build
    build.build()
    return mp.Lib(_abi.LIB_PATH)


@pytest.fixture(scope='module')
def sources():
    return mp.pjpeg_sources()


def test_fixture_covers_the_required_ground(lib, sources):
    import hashlib
    assert mp.PJPEG['parsers'] == (PARSER,) and mp.PJPEG['later']
    assert sorted(sources) == SOURCES and len(SOURCES) == 16
    for geo in ('24x40_420/', '17x33_444/'):
        assert sorted(n[len(geo):] for n in SOURCES if n.startswith(geo)) == [
            'bands', 'ids_2_3', 'pillow', 'ri1', 'ri5', 'shared_tables', 'stops_at_al1']
    assert 'gray/64_scans' in SOURCES and sum(n.startswith('baseline/') for n in SOURCES) == 1
    for name, data in sources.items():   # the regenerated inputs are the recorded ones
        assert hashlib.sha256(data).hexdigest() == PINS['sources'][name], name
        assert len(data) < mp.MAX_SOURCE_BYTES
        # the segments between the scans are mutated: every scan after the first has an SOS at least
        later = mp.later_segments(lib, data)
        if name.startswith('baseline/'):
            assert later == []
        else:
            assert len(later) >= 10 * (data.count(b'\xff\xda') - 1) > 0 and min(later) > mp.first_sos_end(data)
    assert len(mp.GROUPS) == 18 and len(PINS['digests']) == len(SOURCES) * len(mp.GROUPS)
    assert os.path.getsize(mp.PJPEG_PINS) < 100 * 1024


def _first_difference(data, group, got):
    """With JDS_PINS_REF_LIB naming the older build the group is derived again from it and the
    first differing line is returned; without it only this build's lines are at hand."""
    ref = os.environ.get('JDS_PINS_REF_LIB')
    if not ref:
        return 'first lines now: %r (set JDS_PINS_REF_LIB to the older build for the differing line)' % got[:3]
    exp = mp.group_lines(mp.Lib(ref), PARSER, data, group, True)
    for i, (a, b) in enumerate(zip(exp, got)):
        if a != b:
            return 'line %d: recorded %r, now %r' % (i, a, b)
    return 'line counts: recorded %d, now %d' % (len(exp), len(got))


@pytest.mark.parametrize('name', SOURCES)
def test_mutations_and_truncations_answer_as_recorded(lib, sources, name):
    data = sources[name]
    for group in mp.GROUPS:
        got = mp.group_lines(lib, PARSER, data, group, True)
        key = '%s|%s|%s' % (name, PARSER, group)
        if mp.digest(got) != PINS['digests'][key]:
            what = _first_difference(data, group, got)
            print(key, what)
            pytest.fail('%s: %s' % (key, what))


def test_double_defects_report_what_the_parser_reported(lib):
    import ctypes as C
    cases = mp.pjpeg_double_defects()
    assert sorted(cases) == sorted(PINS['double_defects']) and len(cases) == 6
    for name, data in cases.items():
        buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
        assert list(lib.answer(PARSER, buf, len(data))) == PINS['double_defects'][name][PARSER], name
    # the order this parser is known by
    dd = {k: v[PARSER] for k, v in PINS['double_defects'].items()}
    assert 'spectral selection 6..5' in dd['sos_ss_above_se_and_al_14'][1]
    assert 'AC scan with Ns = 3' in dd['ac_scan_ns3_names_an_undefined_table'][1]
    assert 'a refinement has Al = Ah - 1' in dd['refinement_before_first_pass_with_wrong_ah'][1]
    assert dd['scan_65_also_malformed'] == [-2, 'more than 64 scans']
    assert 'bad DHT table header 0x24' in dd['dht_bad_header_and_oversubscribed'][1]
    assert 'sample precision 12' in dd['sof2_precision_12_and_4_components'][1]
