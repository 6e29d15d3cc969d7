#!/bin/bash
# builds nodey-audio-editor_amd/variants/libnae_gpu_stamps.so: the product build (tools/mkvariant.sh), with kernels_pvpipe.hip replaced by a copy
# in which every marked barrier ( /*A*/, /*B*/ ) is stamped with s_memtime (tools/pipe_stamps/stamps.inc).  Diagnostic only.
set -e
HERE=$(cd "$(dirname "$0")" && pwd)
D=$HERE/../../nodey-audio-editor_amd
SRC=$D/csrc/kernels_pvpipe_stamped.hip
trap 'rm -f "$SRC"' EXIT
python3 - "$D/csrc/kernels_pvpipe.hip" "$HERE/stamps.inc" "$SRC" <<'PY'
import re, sys
src, inc, dst = sys.argv[1:4]
s = open(src).read()
s = re.sub(r"pipe_barrier\(\);\s*/\*A\*/", "PIPE_STAMP_BARRIER(t, 0);", s)
s = re.sub(r"pipe_barrier\(\);\s*/\*B\*/", "PIPE_STAMP_BARRIER(t, 1);", s)
s = s.replace("/*pipe:begin*/", "PIPE_TOTAL_BEGIN").replace("/*pipe:r1-end*/", "PIPE_TOTAL_END")
# the scaffolding goes behind pipe_barrier()'s definition
k = s.index("// Issue priority")
s = s[:k] + "} // namespace nae\n" + open(inc).read() + "namespace nae {\n" + s[k:]
open(dst, "w").write(s)
PY
SRC_PVPIPE=$SRC "$HERE/../mkvariant.sh" stamps
