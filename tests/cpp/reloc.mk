# Builds reloc_args_main: the host side of csrc/reloc.hip's entry points (argument checks, block
# carving) with the library's -ffp-contract=off, under the host sanitizers.  The HIP runtime is not
# linked: the few runtime names the host code refers to are defined by the program itself.
#   make -C tests/cpp -f reloc.mk
PKG := ../../orb-slam2-annotation_amd
HIPCC ?= /opt/rocm/bin/hipcc

reloc_args_main: reloc_args_main.cpp $(PKG)/csrc/reloc.hip $(PKG)/csrc/ransac_device.h $(PKG)/csrc/host_common.h \
                 ../../include/orbgpu_reloc.h
	$(HIPCC) -x hip --cuda-host-only -no-hip-rt -O2 -std=c++17 -Wall -ffp-contract=off -fno-fast-math -I../../include \
	    -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ reloc_args_main.cpp

clean:
	rm -f reloc_args_main
.PHONY: clean
