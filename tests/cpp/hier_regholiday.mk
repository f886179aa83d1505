# builds the two checkers of the hierarchical regression holiday, the way Makefile and regholiday.mk build
# theirs (a makefile of its own: Makefile's rules stay as they are):
#   build/ssg_hier_regholiday_check  the host arithmetic (tests/test_ss_hier_regholiday_cpu.py): the header with
#                                    plain g++ and the sanitizers, a program of its own
#   build/libhier_probe.so           the draw kernel, launched directly (tests/test_hier_draw_probe_gpu.py): the
#                                    product's hier_holiday_kernel.hip with the product's flags; nothing of the
#                                    product library is linked
#     make -C tests/cpp -f hier_regholiday.mk
ROOT := ../..
ROCM ?= /opt/rocm
HIPCC ?= $(ROCM)/bin/hipcc
ARCH  ?= gfx950
CSRC := $(ROOT)/boom_amd/csrc
PRODUCT_FLAGS := $(shell sed -n 's/^FLAGS *:= *//p' $(CSRC)/Makefile | sed 's/\$$(ARCH)/$(ARCH)/')

all: build/ssg_hier_regholiday_check build/libhier_probe.so

build/ssg_hier_regholiday_check: ssg_hier_regholiday_check.cpp $(addprefix $(CSRC)/,ssg_regholiday.h kalman_params.h ssvs_params.h) \
                                 $(ROOT)/include/boom_amd.h hier_regholiday.mk
	@mkdir -p build
	g++ -std=c++17 -O1 -g -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    -static-libasan -static-libubsan -D__HIP_PLATFORM_AMD__ -I$(ROCM)/include ssg_hier_regholiday_check.cpp -o $@

HIER_PROBE_DEPS := $(addprefix $(CSRC)/,hier_holiday_kernel.hip mvn_wishart_device.h device_rng.h wave_lanes.h kalman_params.h \
                     ssvs_params.h ktimer.h)
build/libhier_probe.so: hier_probe.hip $(HIER_PROBE_DEPS) $(CSRC)/Makefile hier_regholiday.mk
	@mkdir -p build
	$(HIPCC) $(PRODUCT_FLAGS) -I$(CSRC) -shared hier_probe.hip -o $@

.PHONY: all
