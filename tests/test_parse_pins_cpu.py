"""The two exported parse calls against tests/golden/parse_pins.json (no GPU): the return code,
the message and the struct bytes of jds_jfif_parse and jds_jpeg_parse on small files of every
kind the library reads, on every header byte of them set to each of sixteen values, and on
their truncations; and the named files with two defects in one segment, whose report depends
on the order of a profile's checks.  The fixture was recorded from the build before the two
parsers became one marker walk (tests/golden/make_parse_pins.py), never from the code under
test: both profiles must answer as they did."""
import importlib.util
import json
import os

import pytest

from conftest import ROOT

_spec = importlib.util.spec_from_file_location(
    'make_parse_pins', os.path.join(ROOT, 'tests', 'golden', 'make_parse_pins.py'))
mp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mp)

PINS = json.load(open(mp.PINS))
SOURCES = sorted(PINS['sources'])


@pytest.fixture(scope='module')
def lib():
    from jds import _abi, build
    build.build()
    return mp.Lib(_abi.LIB_PATH)


@pytest.fixture(scope='module')
def sources():
    return mp.sources()


def test_fixture_covers_the_required_ground(sources):
    import hashlib
    assert sorted(sources) == SOURCES and len(SOURCES) == 17
    assert sum(n.startswith('golden/') for n in SOURCES) == 8
    for name, data in sources.items():   # the regenerated inputs are the recorded ones
        assert hashlib.sha256(data).hexdigest() == PINS['sources'][name], name
        assert len(data) < mp.MAX_SOURCE_BYTES
    assert len(mp.GROUPS) == 18 and len(PINS['digests']) == len(SOURCES) * len(mp.PARSERS) * len(mp.GROUPS)
    assert os.path.getsize(mp.PINS) < 100 * 1024


def _first_difference(parser, data, group, got):
    """With JDS_PINS_REF_LIB naming the older build the group is derived again from it and the
    first differing line is returned; without it only this build's lines are at hand."""
    ref = os.environ.get('JDS_PINS_REF_LIB')
    if not ref:
        return 'first lines now: %r (set JDS_PINS_REF_LIB to the older build for the differing line)' % got[:3]
    exp = mp.group_lines(mp.Lib(ref), parser, data, group)
    for i, (a, b) in enumerate(zip(exp, got)):
        if a != b:
            return 'line %d: recorded %r, now %r' % (i, a, b)
    return 'line counts: recorded %d, now %d' % (len(exp), len(got))


@pytest.mark.parametrize('name', SOURCES)
def test_mutations_and_truncations_answer_as_recorded(lib, sources, name):
    data = sources[name]
    for parser in mp.PARSERS:
        for group in mp.GROUPS:
            got = mp.group_lines(lib, parser, data, group)
            key = '%s|%s|%s' % (name, parser, group)
            if mp.digest(got) != PINS['digests'][key]:
                what = _first_difference(parser, data, group, got)
                print(key, what)
                pytest.fail('%s: %s' % (key, what))


def test_double_defects_report_what_each_profile_reported(lib):
    import ctypes as C
    cases = mp.double_defects()
    assert sorted(cases) == sorted(PINS['double_defects']) and len(cases) == 9
    for name, data in cases.items():
        buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
        for parser in mp.PARSERS:
            assert list(lib.answer(parser, buf, len(data))) == PINS['double_defects'][name][parser], (name, parser)
    # the orders the two profiles are known by
    dd = PINS['double_defects']
    assert 'spectral' in dd['sos_bad_spectral_and_table_ids_2_2']['jfif'][1]
    assert 'table ids 2/2' in dd['sos_bad_spectral_and_table_ids_2_2']['jpeg'][1]
    assert 'two quantisation tables' in dd['sof_tq_5_0_0']['jfif'][1] and 'table id 5' in dd['sof_tq_5_0_0']['jpeg'][1]
    assert 'component 7' in dd['fourth_sos_names_component_7']['jfif'][1]
    assert 'more than three scans' in dd['fourth_sos_names_component_7']['jpeg'][1]
    assert dd['dri_4_own_style_17x23']['jfif'][0] == -2 and dd['dri_4_own_style_17x23']['jpeg'][0] == 0
