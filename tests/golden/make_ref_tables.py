#!/usr/bin/env python3
"""Writes tests/golden/ref_tables.json: what tests/ref_parse.py reads from the reference's C sources (needs them on the
machine).  Data only -- integer tables, names and the outcome of each formula check -- so that tests/test_ref_tables.py,
tests/test_capi.py and tests/test_codec_host.py run where the sources are absent; test_ref_tables.py checks this file
against the sources wherever they are present."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ref_parse     # noqa: E402

if not ref_parse.live():
    sys.exit("needs the reference's sources (ref_parse.REF)")
with open(ref_parse.GOLDEN, "w") as f:
    json.dump(ref_parse.parse_all(), f, separators=(",", ":"))
    f.write("\n")
print("wrote", ref_parse.GOLDEN, os.path.getsize(ref_parse.GOLDEN), "bytes")
