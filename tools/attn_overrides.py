"""Command-line overrides of the attention selection rule for the tools: `--attn NAME=VALUE` (repeatable), NAME one of two_block, fwd64,
bwd64_wide, bwd_1p, xcd_order (acai_attn_set_override; values in include/acai_omr_hip.h: ACAI_ATTN_OV_*).  apply(sys.argv) takes those
options out of the argument list, sets them for the process and returns them as text for a tool's result line."""
from acai_omr_amd import _lib

NAMES = {"two_block": _lib.ATTN_OV_TWO_BLOCK, "fwd64": _lib.ATTN_OV_FWD64, "bwd64_wide": _lib.ATTN_OV_BWD64_WIDE, "bwd_1p": _lib.ATTN_OV_BWD_1P,
         "xcd_order": _lib.ATTN_OV_XCD_ORDER}


def apply(argv):
    said = []
    while "--attn" in argv:
        i = argv.index("--attn")
        name, value = argv[i + 1].split("=")
        _lib.check(_lib.lib().acai_attn_set_override(NAMES[name], int(value)), "acai_attn_set_override")
        said.append(argv[i + 1])
        del argv[i:i + 2]
    return " ".join(said) or "no overrides"
