# usage: bash tools/build_variant.sh NAME [extra hipcc flags]  -> tools/tmp_libs/NAME/libwgsparkl{2,3}d_hip.so of the current tree
# (csrc/build.sh with another output directory; run anything with it through WGS_LIB_DIR=tools/tmp_libs/NAME)
set -e
cd "$(dirname "$0")/.."
name=$1; shift
WGS_OUT_DIR="$PWD/tools/tmp_libs/$name" WGS_EXTRA_FLAGS="$*" bash wgsparkl_amd/csrc/build.sh
echo built tools/tmp_libs/$name
