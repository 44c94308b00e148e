# Build an A/B variant of librsgpu.so from the working tree with extra
# compiler flags (a tool, not the product):
#   bash tools/build_variant.sh NAME "-DFLAG ..."  -> tools/ab/librsgpu_NAME.so
# The kernel files below are recompiled with the flags; every other object of
# the library is the Makefile's own (make print-objs), built as the product's.
set -e -o pipefail
NAME=$1; FLAGS=$2
VARIED="rs_kernels rs_bitsliced rs_tc rs_jit"
cd "$(dirname "$0")/../storage-benchmarks_amd"
D=/tmp/rsgpu_variant_$NAME; mkdir -p $D ../tools/ab
KEPT=""; LINK=""
for o in $(make -s print-objs); do
  n=$(basename $o .o)
  case " $VARIED " in *" $n "*) LINK="$LINK $D/$n.o" ;; *) KEPT="$KEPT $o"; LINK="$LINK $o" ;; esac
done
make -s build/enc_progs.inc build/tc_handlers.inc $KEPT
HF="-O3 -std=c++20 -fconstexpr-steps=50000000 -fPIC --offload-arch=gfx950 -w $FLAGS"
pids=""
for f in $VARIED; do
  /opt/rocm/bin/hipcc $HF -Ibuild -c csrc/$f.hip -o $D/$f.o &
  pids="$pids $!"
done
for p in $pids; do wait $p; done
/opt/rocm/bin/hipcc $HF -shared -o ../tools/ab/librsgpu_$NAME.so $LINK -Wl,-soname,librsgpu.so \
  -Wl,--version-script=csrc/rsgpu.map -L/opt/rocm/lib -lhsa-runtime64
echo "built tools/ab/librsgpu_$NAME.so"
