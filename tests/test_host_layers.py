"""The layers of the library's host side (causalgpslc.jl_amd/csrc) depend on each other in one direction only:

    api_predict.hip, api_score.hip -> request.h -> predict.h -> factor.h -> host_ctx.h -> dev_mem.h, gpslc_internal.h

Read from the #include "..." lines of the host sources and headers, and from nothing else: factor.hip includes neither predict.h
nor request.h, predict.hip does not include request.h, api.hip includes none of the three, the two entry-point files do not
include each other, no header of a layer includes one of a layer above it, and each of the four headers has a user other than its
own source."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "causalgpslc.jl_amd", "csrc")

# layer of every host file, bottom first; a file may include host files of its own layer's header and below
LAYER = {"host_ctx.h": 0, "api.hip": 0, "factor.h": 1, "factor.hip": 1, "predict.h": 2, "predict.hip": 2, "request.h": 3,
         "api_predict.hip": 4, "api_score.hip": 4}
OWN_SOURCE = {"host_ctx.h": "api.hip", "factor.h": "factor.hip", "predict.h": "predict.hip", "request.h": "api_predict.hip"}


def includes(name):
    with open(os.path.join(CSRC, name)) as f:
        return {os.path.basename(m.group(1)) for m in (re.match(r'\s*#\s*include\s+"([^"]+)"', line) for line in f) if m}


def test_the_forbidden_includes_are_absent():
    assert not includes("factor.hip") & {"predict.h", "request.h"}
    assert "request.h" not in includes("predict.hip")
    assert not includes("api.hip") & {"factor.h", "predict.h", "request.h"}
    assert "api_score.hip" not in includes("api_predict.hip") and "api_predict.hip" not in includes("api_score.hip")


def test_every_include_points_down():
    for name, layer in LAYER.items():
        for inc in includes(name) & set(LAYER):
            assert inc.endswith(".h"), (name, inc)                      # no source is included
            assert LAYER[inc] <= layer and inc != name, (name, inc)     # a header of its own layer or below
    # what lies under the host layers (kernels, device and shared headers) knows none of them
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".h", ".hip")) and name not in LAYER:
            assert not includes(name) & set(LAYER), name


def test_every_layer_header_has_a_user_beside_its_own_source():
    for header, source in OWN_SOURCE.items():
        users = [n for n in LAYER if n not in (header, source) and header in includes(n)]
        assert users, header
