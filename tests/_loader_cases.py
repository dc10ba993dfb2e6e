"""Scene texts that pin the loader to the reference's own Scene::Load, one rule per case.

CASES maps a name to the file's bytes.  tests/golden/make_golden_loader.py runs the unmodified
reference's parse on each (ref_harness parse) and records the dump and the stderr lines in
tests/golden/loader_cases.json; tests/test_loader_host.py holds the library's parse and the CPU
restatement's against them byte for byte.  RENDERED names the few that are also rendered.

What the fixtures leave out.  The reference gives a Primitive's type, position and shape vectors,
and the temporaries a type line reads into, no initial value: where no line of the file writes
them, what they hold is the stack's, not Scene::Load's (a block without a type line that follows a
BOX block dumps as a copy of that box; a type line too short for its values takes the missing ones
from whatever lay there; a type line resets the position to such a leftover).  unset_words() below
names those words of a dump from the text alone; the generator zeroes them in the fixture, and the
tests zero them in the library's and the restatement's dump before comparing.  Everything a line
wrote -- the failing value of a poisoned or overflowing line included -- is compared.  The rendered
cases give every primitive a type line that reads all its values and a POSITION line after it.
"""

HEAD = b"DIMENSIONS 12 8\nSAMPLES 2\nRAY_DEPTH 3\n"


def _float_text(tok):
    """`tok` first, in the middle and last on a line, at the top level and in a block, each line
    after one that set the three values: an extraction that fails shows in what stays."""
    t = tok if isinstance(tok, bytes) else tok.encode()
    return b"".join([
        HEAD,
        b"BG_COLOR 7 8 9\nBG_COLOR ", t, b" 0.25 0.5\n",
        b"CAMERA_POSITION 7 8 9\nCAMERA_POSITION 0.25 ", t, b" 0.5\n",
        b"CAMERA_UP 7 8 9\nCAMERA_UP 0.25 0.5 ", t, b"\n",
        b"CAMERA_FOV_X 1.5\nCAMERA_FOV_X ", t, b"\n",
        b"NEW_PRIMITIVE\nBOX 1 2 3\n",
        b"COLOR 7 8 9\nCOLOR ", t, b" 0.5 0.25\n",
        b"POSITION 7 8 9\nPOSITION 0.5 ", t, b" 0.25\n",
        b"EMISSION 7 8 9\nEMISSION 0.5 0.25 ", t, b"\n",
        b"ROTATION 1 2 3 4\nROTATION 0.5 0.25 0.125 ", t, b"\n",
        b"IOR 1.5\nIOR ", t, b"\n",
    ])


def _unsigned_text(tok):
    t = tok.encode()
    return b"".join([
        HEAD,
        b"DIMENSIONS ", t, b" 9\n",
        b"SAMPLES ", t, b"\n",
        b"RAY_DEPTH ", t, b"\n",
        b"DIMENSIONS 10 ", t, b"\n",
        b"DIMENSIONS 10 ", t, b" 11\n",
    ])


def _long(n, exponent):
    """a float token of exactly n characters whose value is 1 (with exponent) or 1.5"""
    if not exponent:
        tok = "1.5" + "0" * (n - 3)
    else:
        # 0.000...01e<k + 1> with k zeros after the point: the exponent's digits count too
        for k in range(n):
            tok = "0." + "0" * k + "1e%d" % (k + 1)
            if len(tok) == n:
                break
        else:
            raise AssertionError(n)
    assert len(tok) == n
    return tok


FLOAT_TOKENS = {
    # overflow: the reference stores +-FLT_MAX and fails the line
    "overflow_1e50": "1e50", "overflow_3.5e38": "3.5e38", "overflow_neg_1e39": "-1e39", "overflow_pos_sign": "+1e39",
    "overflow_130_digits": "9" * 130, "overflow_neg_130_digits": "-" + "9" * 130,
    # the largest finite value, decimals just below and above the rounding boundary to 2^128 (FLT_MAX +
    # half an ulp = 340282356779733661637539395458142568448), and the boundary itself
    "flt_max": "3.4028235e38", "flt_max_below_half": "3.4028235677973366e38",
    "flt_max_above_half": "3.4028235677973367e38", "flt_max_half_exact": "340282356779733661637539395458142568448",
    "flt_max_next": "3.4028236e38",
    # underflow: to 0, to a denormal, the smallest denormal and half of it
    "underflow_1e-50": "1e-50", "underflow_neg_1e-50": "-1e-50", "denormal_1e-40": "1e-40", "denormal_min": "1.4e-45",
    "denormal_half_min": "7e-46", "denormal_above_half_min": "7.1e-46", "flt_min": "1.17549435e-38",
    # the one-multiply fast path's edges (scene_load.cpp fast_float): significand 2^24 and 2^24 + 1,
    # 9 and 10 significant digits, powers of ten 10 and 11 either way
    "fast_2p24": "16777216", "fast_2p24_plus1": "16777217", "fast_2p24_plus1_frac": "1677721.7", "fast_9_digits": "123456789",
    "fast_10_digits": "1234567890", "fast_9_digits_frac": "0.123456789", "fast_10_digits_frac": "0.1234567891",
    "fast_e10": "1e10", "fast_e11": "1e11", "fast_em10": "1e-10", "fast_em11": "1e-11", "fast_2p24_e10": "16777216e10",
    "fast_2p24m1_em10": "16777215e-10", "fast_frac_em10": "1234.5678e-6", "fast_frac_em11": "1234.5678e-7",
    "fast_tenth_as_float": "0.100000001490116", "fast_leading_zeros": "000001.5", "fast_leading_zero_frac": "0.000001",
    "fast_many_leading_zeros": "0" * 40 + "7.25", "fast_e0005": "1e0005", "fast_em0005": "1e-0005", "fast_zero_e": "0e5",
    "fast_neg_zero": "-0", "fast_neg_zero_frac": "-0.0", "fast_trailing_zeros": "2.5000000000000", "fast_0.3": "0.3",
    "fast_halfway": "16777217e0", "fast_8388608.5": "8388608.5", "fast_33554434": "33554434",
    # exponents above 1000, and beyond an int
    "exp_1001": "1e1001", "exp_neg_1001": "1e-1001", "exp_zero_5000": "0e5000", "exp_zero_neg_5000": "0.0e-5000",
    "exp_huge": "1e99999999999", "exp_neg_huge": "1e-99999999999", "exp_cancels": "0." + "0" * 1100 + "1e1101",
    "exp_cancels_big": "1" + "0" * 1100 + "e-1100",
    # forms
    "form_inf": "inf", "form_nan": "nan", "form_neg_inf": "-inf", "form_INF": "INF", "form_infinity": "infinity",
    "form_hex": "0x10", "form_1e": "1e", "form_1e_plus": "1e+", "form_1e_minus": "1e-", "form_1.2.3": "1.2.3",
    "form_1-2": "1-2", "form_1+2": "1+2", "form_minus_minus": "--1", "form_plus_minus": "+-1", "form_plus_.5": "+.5",
    "form_minus_.5": "-.5", "form_dot": ".", "form_dot_e5": ".e5", "form_5_dot": "5.", "form_1.e2": "1.e2",
    "form_comma": "1,5", "form_1d5": "1d5", "form_1f": "1f", "form_1e5e3": "1e5e3", "form_1E_plus_2": "1E+2",
    "form_plus": "+", "form_minus": "-", "form_e5": "e5", "form_1e_plus_minus": "1e+-2", "form_1_e5": "1 e5",
    "form_1e5.5": "1e5.5", "form_1e5_minus": "1e5-", "form_nul": "1\x002", "form_high_byte": "1\xe92",
    "form_quote": "1'000", "form_underscore": "1_0", "form_1e_space_5": "1e 5", "form_plus_dot": "+.", "form_p_exp": "1p3",
}
for _n in (127, 128, 129, 300):
    FLOAT_TOKENS["long_%d" % _n] = _long(_n, False)
    FLOAT_TOKENS["long_%d_exp" % _n] = _long(_n, True)
FLOAT_TOKENS["long_1200"] = _long(1200, False)

UNSIGNED_TOKENS = {
    "neg_5": "-5", "plus_7": "+7", "007": "007", "max": "4294967295", "max_plus1": "4294967296",
    "neg_max": "-4294967295", "neg_max_plus1": "-4294967296", "23_digits": "12345678901234567890123", "1.5": "1.5",
    "1e2": "1e2", "hex": "0x1f", "plus": "+", "minus": "-", "neg_0": "-0", "neg_1": "-1", "2p63": "9223372036854775808",
    "2p64": "18446744073709551616", "2p64_minus1": "18446744073709551615", "neg_23_digits": "-12345678901234567890123",
    "leading_zeros_max_plus1": "0004294967296", "letters": "abc", "comma": "1,000", "neg_2p31": "-2147483648",
}

CASES = {}
for _k, _t in FLOAT_TOKENS.items():
    CASES["float_" + _k] = _float_text(_t.encode("latin-1"))
for _k, _t in UNSIGNED_TOKENS.items():
    CASES["unsigned_" + _k] = _unsigned_text(_t)

_BOX = b"NEW_PRIMITIVE\nBOX 1 2 3\nPOSITION 4 5 6\nCOLOR 0.5 0.25 0.125\n"

CASES.update({
    # overflow at given places of the longer lines
    "overflow_triangle_4th": HEAD + b"NEW_PRIMITIVE\nTRIANGLE 1 2 3 1e50 5 6 7 8 9\nCOLOR 1 1 1\n",
    "overflow_triangle_9th": HEAD + b"NEW_PRIMITIVE\nTRIANGLE 1 2 3 4 5 6 7 8 -1e50\nCOLOR 1 1 1\n",
    "overflow_triangle_1st": HEAD + b"NEW_PRIMITIVE\nTRIANGLE 1e39 2 3 4 5 6 7 8 9\nPOSITION 1 2 3\n",
    "overflow_rotation_4th": HEAD + b"NEW_PRIMITIVE\nBOX 1 1 1\nROTATION 0.5 0.5 0.5 1e39\n",
    "overflow_rotation_2nd": HEAD + b"NEW_PRIMITIVE\nBOX 1 1 1\nROTATION 0.5 -4e38 0.5 0.5\n",
    "overflow_ior": HEAD + b"NEW_PRIMITIVE\nBOX 1 1 1\nDIELECTRIC\nIOR 1e39\n",
    "overflow_fov": HEAD + b"CAMERA_FOV_X 1.25\nCAMERA_FOV_X 1e39\n",
    "overflow_box": HEAD + b"NEW_PRIMITIVE\nBOX 1 1e39 3\n",
    "overflow_then_next_line": HEAD + b"BG_COLOR 1e39 2 3\nCAMERA_POSITION 4 5 6\n",
    # lines and blocks
    "crlf": (HEAD + b"BG_COLOR 0.1 0.2 0.3\nCAMERA_POSITION 0 1 5\n\n" + _BOX + b"\nNEW_PRIMITIVE\nELLIPSOID 1 1 1\nMETALLIC\n"
             b"IOR 1.5\n").replace(b"\n", b"\r\n"),
    "crlf_lone_cr_in_block": HEAD + b"NEW_PRIMITIVE\r\nBOX 1 2 3\r\n\r\nCOLOR 1 1 1\r\nPOSITION 1 2 3\r\n\r\nBG_COLOR 1 2 3\r\n",
    "cr_only": HEAD.replace(b"\n", b"\r") + b"BG_COLOR 1 2 3\r",
    "separators_vt_ff_tab": b"DIMENSIONS\t12\v8\nSAMPLES\f2\nRAY_DEPTH \t 3\n\tBG_COLOR\v0.1\f0.2\t0.3\n \vNEW_PRIMITIVE\n\fBOX\t1\v2\f3\n"
                            b"\t POSITION 4\t\t5 \v 6\n",
    "leading_spaces": b"   DIMENSIONS   12   8   \n  NEW_PRIMITIVE  \n   BOX 1 2 3\n   \n  SAMPLES 4\n",
    "no_final_newline": HEAD + b"NEW_PRIMITIVE\nBOX 1 2 3\nCOLOR 0.5 0.25 0.125",
    "no_final_newline_top": HEAD + b"BG_COLOR 0.5 0.25 0.125",
    "empty": b"",
    "only_newlines": b"\n\n\n",
    "only_spaces": b"   \n \t \n",
    "ends_inside_block": HEAD + b"NEW_PRIMITIVE\nBOX 1 2 3\n",
    "ends_after_new_primitive": HEAD + b"NEW_PRIMITIVE\n",
    "ends_after_new_primitive_no_newline": HEAD + b"NEW_PRIMITIVE",
    "blank_line_ends_block": HEAD + b"NEW_PRIMITIVE\nBOX 1 2 3\n\nCOLOR 1 1 1\nPOSITION 1 1 1\n",
    "spaces_line_ends_block": HEAD + b"NEW_PRIMITIVE\nBOX 1 2 3\n  \t \nIOR 2\nMETALLIC\n",
    "new_primitive_in_block": HEAD + b"NEW_PRIMITIVE\nBOX 1 2 3\nCOLOR 1 0 0\nNEW_PRIMITIVE\nELLIPSOID 4 5 6\nCOLOR 0 1 0\n"
                              b"NEW_PRIMITIVE 1 2\nPLANE 0 1 0\n",
    "new_primitive_twice": HEAD + b"NEW_PRIMITIVE\nNEW_PRIMITIVE\nBOX 1 2 3\n",
    "two_type_lines": HEAD + b"NEW_PRIMITIVE\nBOX 1 2 3\nCOLOR 1 0.5 0.25\nEMISSION 1 2 3\nPOSITION 4 5 6\nROTATION 0.5 0.5 0.5 0.5\n"
                      b"METALLIC\nIOR 1.5\nELLIPSOID 7 8 9\nPOSITION 0.5 0.25 0.125\n",
    "two_type_lines_triangle_then_box": HEAD + b"NEW_PRIMITIVE\nTRIANGLE 1 2 3 4 5 6 7 8 9\nCOLOR 1 0.5 0.25\nBOX 3 2 1\nIOR 2\n",
    "metallic_then_dielectric": HEAD + b"NEW_PRIMITIVE\nBOX 1 2 3\nPOSITION 1 2 3\nMETALLIC\nDIELECTRIC\nIOR 1.5\n\nNEW_PRIMITIVE\nELLIPSOID 1 1 1\n"
                                b"POSITION 3 2 1\nDIELECTRIC\nMETALLIC\n",
    "material_with_arguments": HEAD + b"NEW_PRIMITIVE\nBOX 1 2 3\nMETALLIC 5 6\nIOR\n",
    "position_before_type": HEAD + b"NEW_PRIMITIVE\nPOSITION 4 5 6\nCOLOR 1 1 1\nDIELECTRIC\nIOR 1.5\nROTATION 0 0 1 0\nEMISSION 1 1 1\n"
                            b"BOX 1 2 3\n",
    "no_type_line": HEAD + b"NEW_PRIMITIVE\nCOLOR 1 0.5 0.25\nPOSITION 4 5 6\nIOR 1.25\n",
    "short_lines_3": HEAD + b"BG_COLOR 7 8 9\nBG_COLOR 1 2\nCAMERA_POSITION 7 8 9\nCAMERA_POSITION 1\nCAMERA_RIGHT 7 8 9\nCAMERA_RIGHT\n"
                     b"CAMERA_UP 7 8 9\nCAMERA_UP 1 2 \nCAMERA_FORWARD 7 8 9\nCAMERA_FORWARD   \n"
                     b"NEW_PRIMITIVE\nBOX 1 2 3\nCOLOR 7 8 9\nCOLOR 1 2\nPOSITION 7 8 9\nPOSITION 1\nEMISSION 7 8 9\nEMISSION\n",
    "short_lines_4": HEAD + b"NEW_PRIMITIVE\nBOX 1 2 3\nROTATION 5 6 7 8\nROTATION 1 2 3\n\nNEW_PRIMITIVE\nBOX 1 2 3\nROTATION 1\n\n"
                     b"NEW_PRIMITIVE\nBOX 1 2 3\nROTATION\n",
    "short_box": HEAD + b"NEW_PRIMITIVE\nBOX 1 2\n",
    "short_ellipsoid": HEAD + b"NEW_PRIMITIVE\nELLIPSOID 1\n",
    "short_plane": HEAD + b"NEW_PRIMITIVE\nPLANE\n",
    "short_triangle_8": HEAD + b"NEW_PRIMITIVE\nTRIANGLE 1 2 3 4 5 6 7 8\n",
    "short_triangle_0": HEAD + b"NEW_PRIMITIVE\nTRIANGLE\nCOLOR 1 0.5 0.25\n",
    "short_triangle_4": HEAD + b"NEW_PRIMITIVE\nTRIANGLE 1 2 3 4\n",
    "short_scalars": HEAD + b"CAMERA_FOV_X 1.5\nCAMERA_FOV_X\nDIMENSIONS 5\nDIMENSIONS\nSAMPLES\nRAY_DEPTH \nNEW_PRIMITIVE\nBOX 1 2 3\n"
                     b"IOR 1.5\nIOR\n",
    "extra_values": HEAD + b"BG_COLOR 1 2 3 4 5\nDIMENSIONS 3 4 5\nNEW_PRIMITIVE\nBOX 1 2 3 4\nPOSITION 4 5 6 7\nROTATION 1 2 3 4 5\nIOR 1 2\n",
    "poisoned_line": HEAD + b"BG_COLOR 7 8 9\nBG_COLOR 1 x 3\nNEW_PRIMITIVE\nBOX 1 2 3\nCOLOR 7 8 9\nCOLOR x 2 3\nPOSITION 7 8 9\n"
                     b"POSITION 1 2 x\n",
    "poisoned_type_line": HEAD + b"NEW_PRIMITIVE\nBOX 1 x 3\nCOLOR 1 1 1\n",
    "unknown_top_level": HEAD + b"FOO 1 2 3\nbar\nBG_COLOR 1 2 3\n#comment\nDIMENSION 5 5\n",
    "unknown_in_block": HEAD + b"NEW_PRIMITIVE 0.5 0.25\nBOX 1 2 3\nFOO 1 2 3\nCOLOR 1 1 1\n",
    "command_with_trailing_cr": HEAD + b"NEW_PRIMITIVE\r\nBOX 1 2 3\nMETALLIC\r\nCOLOR 1 1 1\nDIELECTRIC\r\n",
    "new_primitive_with_trailing_cr_only": b"DIMENSIONS 12 8\r\nNEW_PRIMITIVE\r\nBOX 1 2 3\r\n",
    "lower_case": b"dimensions 12 8\nDimensions 12 8\nNEW_PRIMITIVE\nbox 1 2 3\nCOLOR 1 1 1\n",
    "lower_case_new_primitive": HEAD + b"new_primitive\nBOX 1 2 3\n",
    "command_prefixes": HEAD + b"BG_COLOR2 1 2 3\nBG_COLO 1 2 3\nCAMERA_FOV_Y 2\nNEW_PRIMITIVES\nNEW_PRIMITIVE\nBOX 1 2 3\nBOXX 1 2 3\n",
    "block_commands_at_top_level": HEAD + b"BOX 1 2 3\nCOLOR 1 1 1\nMETALLIC\nIOR 2\nPOSITION 1 2 3\nTRIANGLE 1 2 3 4 5 6 7 8 9\n",
    "nul_bytes": HEAD + b"BG_COLOR 1 2 3\n\x00\nNEW_PRIMITIVE\nBOX 1 2 3\n\x00COLOR 1 1 1\nCOLOR\x00 1 1 1\n",
    "high_bytes": HEAD + b"\xff\xfe 1\nNEW_PRIMITIVE\nBOX 1 2 3\nCOLOR\xa0 1 1 1\n\xa0\nPOSITION 1 2 3\n",
    "bom": b"\xef\xbb\xbfDIMENSIONS 12 8\nSAMPLES 2\n",
    "every_command": HEAD + b"BG_COLOR 0.1 0.2 0.3\nCAMERA_POSITION 1 2 3\nCAMERA_RIGHT 4 5 6\nCAMERA_UP 7 8 9\nCAMERA_FORWARD 10 11 12\n"
                     b"CAMERA_FOV_X 1.25\nNEW_PRIMITIVE\nPLANE 0 1 0\nPOSITION 0 -1 0\nCOLOR 0.5 0.5 0.5\nNEW_PRIMITIVE\nELLIPSOID 1 2 3\nPOSITION 1 0 0\n"
                     b"ROTATION 0.1 0.2 0.3 0.4\nEMISSION 5 6 7\nNEW_PRIMITIVE\nBOX 1 2 3\nPOSITION 0 2 0\nDIELECTRIC\nIOR 1.5\nNEW_PRIMITIVE\n"
                     b"TRIANGLE 1 2 3 4 5 6 7 8 9\nPOSITION 0 0 3\nMETALLIC\nCOLOR 0.9 0.8 0.7\n",
    "dimensions_repeat": HEAD + b"DIMENSIONS 5 6\nDIMENSIONS 7\nDIMENSIONS x 9\n",
})

# NEW_PRIMITIVE with trailing arguments, then each top-level command that ends the block: it is read
# off the NEW_PRIMITIVE line's stream
for _cmd in ("DIMENSIONS", "BG_COLOR", "CAMERA_POSITION", "CAMERA_RIGHT", "CAMERA_UP", "CAMERA_FORWARD", "CAMERA_FOV_X",
             "RAY_DEPTH", "SAMPLES", "FOO"):
    CASES["stale_stream_" + _cmd] = (HEAD + b"BG_COLOR 0.5 0.5 0.5\nNEW_PRIMITIVE 21 22.5 23 24\nBOX 1 2 3\nPOSITION 4 5 6\n" + _cmd.encode() +
                                     b" 31 32 33\nCAMERA_FOV_X 0.75\n")
CASES["stale_stream_short"] = HEAD + b"NEW_PRIMITIVE 21\nBOX 1 2 3\nBG_COLOR 31 32 33\n"
CASES["stale_stream_empty"] = HEAD + b"BG_COLOR 7 8 9\nNEW_PRIMITIVE\nBOX 1 2 3\nPOSITION 4 5 6\nBG_COLOR 31 32 33\nSAMPLES 5\n"
CASES["stale_stream_poisoned"] = HEAD + b"BG_COLOR 7 8 9\nNEW_PRIMITIVE 1 x 3\nBOX 1 2 3\nBG_COLOR 31 32 33\n"
CASES["stale_stream_overflow"] = HEAD + b"BG_COLOR 7 8 9\nNEW_PRIMITIVE 1e39 2 3\nBOX 1 2 3\nBG_COLOR 31 32 33\n"
CASES["stale_stream_twice"] = (HEAD + b"NEW_PRIMITIVE 21 22 23 24 25\nBOX 1 2 3\nDIMENSIONS 0 0\nNEW_PRIMITIVE 5\nELLIPSOID 1 1 1\n"
                               b"SAMPLES 9\nRAY_DEPTH 9\n")
CASES["stale_stream_unsigned_reads_float"] = HEAD + b"NEW_PRIMITIVE 2.5 7\nBOX 1 2 3\nDIMENSIONS 1 1\n"

# ---- the cases that are also rendered (12 x 8, 2 samples, RAY_DEPTH 3): a wrong parse changes pixels
_ROOM = (b"DIMENSIONS 12 8\nSAMPLES 2\nRAY_DEPTH 3\nBG_COLOR 0.2 0.3 0.4\nCAMERA_POSITION 0 0.5 6\nCAMERA_RIGHT 1 0 0\n"
         b"CAMERA_UP 0 1 0\nCAMERA_FORWARD 0 0 -1\nCAMERA_FOV_X 1.2\n\n"
         b"NEW_PRIMITIVE\nPLANE 0 1 0\nPOSITION 0 -1 0\nCOLOR 0.7 0.7 0.7\n\n"
         b"NEW_PRIMITIVE\nELLIPSOID 0.6 0.6 0.6\nPOSITION 0 3 1\nCOLOR 1 1 1\nEMISSION 9 8 7\n\n")
_L200 = b"1.25" + b"0" * 196
assert len(_L200) == 200
RENDERED = {
    # POSITION's first value overflows: x = FLT_MAX would put the box out of sight; y and z stay what the
    # line before set (read on, they would be 2 and 3)
    "render_position_overflow": _ROOM + b"NEW_PRIMITIVE\nBOX 1 1 1\nCOLOR 0.9 0.2 0.2\nPOSITION 0.5 0.25 0.5\nPOSITION 1e39 2 3\n",
    # the middle value of COLOR overflows: r read, g = FLT_MAX is no case for pixels, so the poisoned
    # line is one whose second token is no number: g and b stay as the line before left them
    "render_color_poisoned": _ROOM + b"NEW_PRIMITIVE\nBOX 1 1 1\nPOSITION 0.25 0 0\nCOLOR 0.1 0.9 0.2\nCOLOR 0.8 x 0.9\n",
    # (a negative overflow in EMISSION's last place was a case here: the reference never returns from
    # rendering an emitter of -FLT_MAX, so it is no fixture)
    # (and one whose ROTATION's 4th value overflows: the reference faults on a rotator of FLT_MAX)
    # \t, \v and \f between the tokens
    "render_separators": _ROOM + b"NEW_PRIMITIVE\nBOX\t1\v0.5\f0.25\n\tCOLOR\v0.5\f0.9\t0.5\n\fPOSITION \t0.5\v\v0 1\n",
    # a 200-character coordinate
    "render_long_coordinate": _ROOM + b"NEW_PRIMITIVE\nBOX 1 1 1\nCOLOR 0.2 0.9 0.2\nPOSITION " + _L200 + b" 0.5 -0.5\n",
    # a 140-character box size with an exponent
    "render_long_size_exp": _ROOM + b"NEW_PRIMITIVE\nBOX 1 " + _long(140, True).encode() + b" 0.5\nPOSITION 0 0.25 0\nCOLOR 0.2 0.2 0.9\n",
    "render_crlf": (_ROOM + b"NEW_PRIMITIVE\nBOX 1 1 1\nCOLOR 0.9 0.9 0.2\nMETALLIC\nPOSITION -0.5 0 0\n").replace(b"\n", b"\r\n"),
    # BG_COLOR ends the block and is read off the NEW_PRIMITIVE line's stream
    "render_stale_bg_color": _ROOM + b"NEW_PRIMITIVE 0.9 0.1 0.1\nBOX 1 1 1\nPOSITION 0 0 0.25\nCOLOR 0.5 0.5 0.5\nBG_COLOR 0 0 0\n",
    # an overflowing FOV is FLT_MAX ... which renders NaN; the IOR of a glass box overflows instead: the
    # line before it stays
    "render_ior_overflow": _ROOM + b"NEW_PRIMITIVE\nBOX 1 1 1\nPOSITION 0 0.25 0.5\nCOLOR 0.9 0.9 0.9\nDIELECTRIC\nIOR 1.5\nIOR 1e39 \n",
}
assert len(RENDERED) <= 8 and not set(RENDERED) & set(CASES)
CASES.update(RENDERED)

for _k, _v in CASES.items():
    assert isinstance(_v, bytes) and len(_v) < 16384, _k


def text_md5(name):
    import hashlib
    return hashlib.md5(CASES[name]).hexdigest()


# ---- the fields of a dump that no line of the file wrote
# (words of the 100-byte primitive record: 0 type, 1-9 the shape vectors, 10-12 position)
_BLOCK = (b"PLANE", b"ELLIPSOID", b"BOX", b"TRIANGLE", b"COLOR", b"POSITION", b"ROTATION", b"METALLIC", b"DIELECTRIC", b"IOR",
          b"EMISSION")
_PLAIN = __import__("re").compile(rb"[+-]?(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?\Z")


def _written(tokens, want):
    """how many of a line's `want` values an extraction writes: the plain finite numbers it reads,
    and the token it fails on (0 or +-FLT_MAX is stored); at the line's end nothing is stored"""
    n = 0
    for t in tokens[:want]:
        n += 1
        if not _PLAIN.match(t) or not abs(float(t)) <= 3.4028234664e38:
            break
    return n


def unset_words(text):
    """Per primitive of `text`, in file order, the record words that the reference leaves to the stack
    (see the module's header): the generator and the tests zero them on both sides.  Conservative: a
    token that is not a plain decimal number counts as the one the line fails on."""
    out, cur, in_block = [], None, False
    for line in text.split(b"\n"):
        tok = line.split()   # (bytes.split: the C locale's whitespace)
        if tok and tok[0] == b"NEW_PRIMITIVE":
            cur, in_block = set(range(0, 13)), True
            out.append(cur)
            continue
        if not in_block:
            continue
        if not tok or tok[0] not in _BLOCK:
            in_block = False
            continue
        if tok[0] in (b"PLANE", b"ELLIPSOID", b"BOX", b"TRIANGLE"):
            want = 9 if tok[0] == b"TRIANGLE" else 3
            cur.clear()
            cur.update(range(1 + _written(tok[1:], want), 1 + want))   # (words 4-9 of the others: dumped as 0)
            cur.update(range(10, 13))                                  # the type line resets the position
        elif tok[0] == b"POSITION":
            cur.difference_update(range(10, 10 + _written(tok[1:], 3)))
    return [sorted(s) for s in out]


def mask_unset(text, dump):
    """`dump` (bytes) with the words of unset_words(text) zeroed"""
    b = bytearray(dump)
    for i, words in enumerate(unset_words(text)):
        for w in words:
            o = 80 + 100 * i + 4 * w
            if o + 4 <= len(b):
                b[o:o + 4] = b"\0\0\0\0"
    return bytes(b)
