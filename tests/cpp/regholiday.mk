# builds the host-only check of the regression holiday's host arithmetic (tests/test_ssg_regholiday_cpu.py),
# the way Makefile builds ssg_spec_check: the headers with plain g++ and the sanitizers.
#     make -C tests/cpp -f regholiday.mk
ROOT := ../..
ROCM ?= /opt/rocm
CSRC := $(ROOT)/boom_amd/csrc

all: build/ssg_regholiday_check

build/ssg_regholiday_check: ssg_regholiday_check.cpp $(addprefix $(CSRC)/,ssg_regholiday.h ssg_instances.h ssg_spec.h kalman_params.h ssvs_params.h student_params.h latent_params.h) \
                            $(ROOT)/include/boom_amd.h regholiday.mk
	@mkdir -p build
	g++ -std=c++17 -O1 -g -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    -static-libasan -static-libubsan -D__HIP_PLATFORM_AMD__ -I$(ROCM)/include ssg_regholiday_check.cpp -o $@

.PHONY: all
