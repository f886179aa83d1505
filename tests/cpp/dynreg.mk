# builds the host-only check of the dynamic regression's part of the state-model list's arithmetic
# (tests/test_ssg_dynreg_cpu.py), the way Makefile builds ssg_spec_check: the header with plain g++ and
# the sanitizers.    make -C tests/cpp -f dynreg.mk
ROOT := ../..
ROCM ?= /opt/rocm
CSRC := $(ROOT)/boom_amd/csrc

all: build/ssg_dynreg_check

build/ssg_dynreg_check: ssg_dynreg_check.cpp $(addprefix $(CSRC)/,ssg_spec.h kalman_params.h ssvs_params.h student_params.h latent_params.h) \
                        $(ROOT)/include/boom_amd.h dynreg.mk
	@mkdir -p build
	g++ -std=c++17 -O1 -g -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    -static-libasan -static-libubsan -D__HIP_PLATFORM_AMD__ -I$(ROCM)/include ssg_dynreg_check.cpp -o $@

.PHONY: all
