#!/bin/bash
# Diagnostic build of the library with phase stamps in the binning pass (-DLNERF_STAMPS); never the product library.
# Compiles the sources of latent-nerf-test_amd/build.py with its flags.
set -eu
R=$(cd "$(dirname "$0")/.." && pwd)
C=$R/latent-nerf-test_amd/csrc
O=$R/latent-nerf-test_amd/lib/stamps
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
mkdir -p $O
build_list() { (cd $R/latent-nerf-test_amd && python3 -B -c "import build; print(' '.join(build.$1))"); }
read -r -a SOURCES <<< "$(build_list SOURCES)"
read -r -a FLAGS <<< "$(build_list FLAGS)"
FLAGS+=(-DLNERF_STAMPS '-DLNERF_BUILD_TAG="stamps"')
objs=() pids=()
for f in "${SOURCES[@]}"; do
  flags=()
  for fl in "${FLAGS[@]}"; do [[ $f == *.cc && $fl == --offload-arch=* ]] || flags+=("$fl"); done   # (host-only, as build.py)
  objs+=("$O/${f%.*}.o")
  $HIPCC "${flags[@]}" -c "$C/$f" -o "${objs[-1]}" &
  pids+=($!)
done
for p in "${pids[@]}"; do wait $p; done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o $R/latent-nerf-test_amd/lib/liblnerf_hip_stamps.so "${objs[@]}"
echo built $R/latent-nerf-test_amd/lib/liblnerf_hip_stamps.so
