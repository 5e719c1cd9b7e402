"""The figures of the C ABI that several test modules pin: one place to move them when the ABI moves."""
VERSION = 108             # simulst_version() == _lib.ABI_VERSION: moves when a descriptor structure or an argument list changes
N_SIGNATURES = 84         # len(_lib.SIGNATURES) == the simulst_* symbols the shipped library exports
LINEAR_DESC_BYTES = 152   # sizeof(simulst_linear_desc)
CTC_PREFIX_DESC_BYTES = 64    # sizeof(simulst_ctc_prefix_desc)
