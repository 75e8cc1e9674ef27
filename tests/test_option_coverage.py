"""Every name lsqr_set_option knows (the rows of kOptions in lsqrrecipes_amd/csrc/options.h) is passed
to set_option by some test, or is listed in EXEMPT below with the reason why not.  Each knob selects another kernel
instantiation, launch shape or host path, and the contract is that no answer depends on one (tests/
test_gpu_option_matrix.py): a knob that arrives without a test fails here.  Runs without a GPU."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "lsqrrecipes_amd", "csrc", "options.h")

# option -> why no test sets it
EXEMPT = {
    "syrk_diag": "timing diagnostics of the dense SYRK (loads only / MFMAs only), documented to give wrong sums",
    "dense_mask_diag": "timing diagnostics of k_mask_syrk_dense (no MFMA / no row evaluation), documented to give wrong results",
    "lm_persist_resident": "persistent-kernel variant that is off by default and measured no faster; whether to keep it is "
                           "a separate decision, and no test launches it",
}


def _option_names():
    with open(SOURCE) as f:
        text = f.read()
    begin = text.index("inline constexpr OptionRow kOptions[] = {")
    end = text.index("\n};", begin)                   # the table's closing brace
    # a row: {"name", &Options::member (nullptr for a removed option), rule, ...
    return re.findall(r'^\s*\{"([A-Za-z0-9_]+)", (?:&Options::\w+|nullptr), OPT_[A-Z_]+,', text[begin:end], re.M)


def _quoted_in_tests():
    me = os.path.abspath(__file__)
    found = set()
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "*.py"))):
        if os.path.abspath(path) == me:              # the keys of EXEMPT are no tests
            continue
        with open(path) as f:
            found.update(re.findall(r"""["']([A-Za-z0-9_]+)["']""", f.read()))
    return found


def test_the_option_list_is_read_from_the_source():
    names = _option_names()
    assert len(names) == len(set(names)), sorted(n for n in names if names.count(n) > 1)
    assert len(names) >= 53                           # (what the source held when this guard was written)
    for known in ("batch_lanes", "scan_ppl", "scan_hsplit", "upload_threads", "dense_dd"):  # first, last and between
        assert known in names


def test_every_option_is_set_by_a_test_or_exempt_with_a_reason():
    quoted = _quoted_in_tests()
    missing = [n for n in _option_names() if n not in quoted and n not in EXEMPT]
    assert not missing, "options no test sets (add a test, or an entry with the reason to EXEMPT): %s" % missing
    for name, reason in EXEMPT.items():
        assert isinstance(reason, str) and len(reason.split()) >= 5, name


def test_every_exemption_is_still_an_option_and_still_needed():
    names = _option_names()
    quoted = _quoted_in_tests()
    for name in EXEMPT:
        assert name in names, "%s is no option any more: drop it from EXEMPT" % name
        assert name not in quoted, "%s is set by a test now: drop it from EXEMPT" % name


def test_the_options_of_the_matrix_need_no_exemption():
    quoted = _quoted_in_tests()
    for name in ("scan_hsplit", "scan_pairs", "scan_hyp_order", "scan_pairs_waves", "scan_presorted", "dense_mask_ring",
                 "upload_threads", "scan_pairs_mfma"):
        assert name in quoted and name not in EXEMPT, name
