"""CPU: the option ledger of tests/options_ref.py against PN2_OPTION_LIST of csrc/pn2_common.h.  No GPU, no library load: the
header is parsed with a regular expression and the test functions the ledger names are looked up in the text of tests/."""
import glob
import os
import re

import options_ref as O

TESTS = os.path.dirname(os.path.abspath(__file__))


def _defined_tests():
    out = set()
    for path in glob.glob(os.path.join(TESTS, "test_*.py")):
        module = os.path.splitext(os.path.basename(path))[0]
        out.update("%s::%s" % (module, name) for name in re.findall(r"^def (test_\w+)\(", open(path).read(), re.M))
    return out


def test_the_header_table_parses_and_every_default_is_an_integer():
    table = O.header_options()
    assert len(table) >= 40 and len({name for name, _ in table}) == len(table), "PN2_OPTION_LIST: too few entries or a repeated name"
    for name, value in table:
        assert re.fullmatch(r"-?\d+", value), "default of %s is not an integer literal: %r" % (name, value)
    assert O.header_defaults()["PN2_FPS_SINGLE_MAX"] == 24576 and O.header_defaults()["PN2_WGRAD_TWO_PHASE"] == 0


def test_every_option_of_the_header_has_a_ledger_entry_and_no_other():
    names = {name for name, _ in O.header_options()}
    missing, stale = sorted(names - set(O.LEDGER)), sorted(set(O.LEDGER) - names)
    assert not missing, "options without a ledger entry (say in tests/options_ref.py where the alternative route is tested): %s" % missing
    assert not stale, "ledger entries of options the header no longer has: %s" % stale


def test_every_ledger_entry_has_one_of_the_stated_forms():
    for name, value in O.LEDGER.items():
        if isinstance(value, str):
            assert re.fullmatch(r"bit-equal pair tested in test_\w+::test_\w+", value), (name, value)
        elif isinstance(value, tuple):
            assert len(value) == 2 and value[0] == "threshold" and isinstance(value[1], str) and value[1], (name, value)
        else:
            pairs = [item for item in value if isinstance(item, tuple)]
            notes = [item for item in value if not isinstance(item, tuple)]
            assert pairs and all(len(p) == 2 and isinstance(p[0], (int, str)) and re.fullmatch(r"test_\w+::test_\w+", p[1]) for p in pairs), (name, value)
            assert all(n in (O.NOTE_GRID, O.NOTE_FPS) for n in notes), (name, notes)
            default = O.header_defaults()["PN2_" + name]
            assert any(p[0] != default for p in pairs), "%s: the ledger lists only the default value" % name


def test_every_test_the_ledger_names_exists():
    unknown = sorted(O.ledger_test_ids() - _defined_tests())
    assert not unknown, "the ledger names tests that do not exist: %s" % unknown


def test_the_parser_sees_an_added_and_a_removed_option(tmp_path):
    """The check of the second test is not vacuous: an option added to (or taken out of) a copy of the header shows."""
    text = open(O.HEADER).read()
    added = tmp_path / "added.h"
    added.write_text(text.replace("    X(FPS_ROWMAP, 2)", "    X(BRAND_NEW, 7) /* new */ \\\n    X(FPS_ROWMAP, 2)", 1))
    names = {name for name, _ in O.header_options(str(added))}
    assert names - set(O.LEDGER) == {"BRAND_NEW"} and O.header_defaults(str(added))["PN2_BRAND_NEW"] == 7
    removed = tmp_path / "removed.h"
    removed.write_text(re.sub(r"    X\(FPS_ROWMAP, 2\)[^\n]*\n", "", text, count=1))
    assert set(O.LEDGER) - {name for name, _ in O.header_options(str(removed))} == {"FPS_ROWMAP"}
