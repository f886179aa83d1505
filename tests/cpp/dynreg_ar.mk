# builds the host-only check of the AR dynamic regression's part of the state-model list's arithmetic
# (tests/test_ss_dynreg_ar_cpu.py), the way dynreg.mk builds ssg_dynreg_check: the headers with plain g++ and
# the sanitizers.    make -C tests/cpp -f dynreg_ar.mk
ROOT := ../..
ROCM ?= /opt/rocm
CSRC := $(ROOT)/boom_amd/csrc

all: build/ssg_dynreg_ar_check

build/ssg_dynreg_ar_check: ssg_dynreg_ar_check.cpp $(addprefix $(CSRC)/,ssg_spec.h ssg_instances.h kalman_params.h ssvs_params.h student_params.h latent_params.h) \
                           $(ROOT)/include/boom_amd.h dynreg_ar.mk
	@mkdir -p build
	g++ -std=c++17 -O1 -g -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    -static-libasan -static-libubsan -D__HIP_PLATFORM_AMD__ -I$(ROCM)/include ssg_dynreg_ar_check.cpp -o $@

.PHONY: all
