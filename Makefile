# Builds the HIP module (C ABI of include/datum_ocean_hip.h) for gfx950, the C++ host shim and the CPU oracle.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
HIPFLAGS ?= -O3 -std=c++17 --offload-arch=$(ARCH) -fPIC -ffp-contract=off -fno-fast-math -Wall -Wno-unused-function

LIB = datum_amd/lib/libdatum_ocean_hip.so
SRC = datum_amd/csrc/ocean_capi.hip
DEPS = datum_amd/csrc/ocean_kernels.hip datum_amd/csrc/ocean_literal.hip datum_amd/csrc/ocean_gen.hip datum_amd/csrc/ocean_farm.hip datum_amd/csrc/ocean_foam.hip datum_amd/csrc/ocean_surface.hip datum_amd/csrc/ocean_query.hip datum_amd/csrc/ocean_blend.hip datum_amd/csrc/ocean_body.hip datum_amd/csrc/ocean_body.h datum_amd/csrc/ocean_ray.hip datum_amd/csrc/ocean_ray.h datum_amd/csrc/ocean_bounds.hip datum_amd/csrc/ocean_bounds.h datum_amd/csrc/ocean_velocity.hip datum_amd/csrc/ocean_velocity.h datum_amd/csrc/ocean_drag.hip datum_amd/csrc/ocean_drag.h datum_amd/csrc/ocean_step.hip datum_amd/csrc/ocean_step.h datum_amd/csrc/ocean_ripple.hip datum_amd/csrc/ocean_ripple.h datum_amd/csrc/ocean_couple.hip datum_amd/csrc/ocean_couple.h datum_amd/csrc/ocean_contact.hip datum_amd/csrc/ocean_contact.h datum_amd/csrc/ocean_rippled.hip datum_amd/csrc/ocean_rippled.h datum_amd/csrc/ocean_ripple_bounds.hip datum_amd/csrc/ocean_ripple_bounds.h datum_amd/csrc/ocean_ripple_foam.hip datum_amd/csrc/ocean_ripple_foam.h datum_amd/csrc/ocean_ripple_deep.hip datum_amd/csrc/ocean_ripple_deep.h datum_amd/csrc/ocean_ripple_wall.hip datum_amd/csrc/ocean_ripple_wall.h datum_amd/csrc/ocean_ripple_bed.hip datum_amd/csrc/ocean_ripple_bed.h datum_amd/csrc/ocean_ripple_swell.hip datum_amd/csrc/ocean_ripple_swell.h $(wildcard datum_amd/csrc/ocean_gen_*.inc) datum_amd/csrc/ocean_fft_core.h datum_amd/csrc/ocean_layout.h datum_amd/csrc/ocean_writeback.h datum_amd/csrc/ocean_phase.h datum_amd/csrc/ocean_quadrant.h include/datum_ocean_hip.h

HOSTLIB = datum_amd/lib/libdatum_ocean_host.so
HOSTSRC = datum_amd/host/ocean.cpp datum_amd/host/host_capi.cpp
HOSTDEPS = datum_amd/host/ocean.h datum_amd/host/lml.h include/datum_ocean_hip.h
CXX ?= g++
HOSTFLAGS ?= -O2 -std=c++14 -fPIC -ffp-contract=off -fno-fast-math -Wall

# measurement aid of bench.py --standin-peers (a CU-occupying stand-in for the all-gather on one GPU); not the ocean path
STANDIN = datum_amd/lib/libdatum_farm_standin.so

all: $(LIB) $(HOSTLIB) $(STANDIN) oracle examples

$(STANDIN): datum_amd/csrc/farm_standin.hip
	@mkdir -p datum_amd/lib
	$(HIPCC) -O3 -std=c++17 --offload-arch=$(ARCH) -fPIC -shared -o $@ datum_amd/csrc/farm_standin.hip

# the C++ host shim links only against the C ABI of the HIP module
$(HOSTLIB): $(HOSTSRC) $(HOSTDEPS) $(LIB)
	$(CXX) $(HOSTFLAGS) -shared -o $@ $(HOSTSRC) -Ldatum_amd/lib -ldatum_ocean_hip -Wl,-rpath,'$$ORIGIN'

$(LIB): $(SRC) $(DEPS)
	@mkdir -p datum_amd/lib
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $(SRC)

oracle:
	$(MAKE) -C oracle liboracle.so

# datum's example-ocean flow against the host shim, headless
EXAMPLE = examples/ocean_headless
FARMEXAMPLE = examples/ocean_farm
examples: $(EXAMPLE) $(FARMEXAMPLE)

# the tile farm from C++ alone (N processes, RCCL through the C ABI)
$(FARMEXAMPLE): examples/ocean_farm.cpp $(HOSTLIB)
	$(CXX) -O2 -std=c++14 -Wall -o $@ examples/ocean_farm.cpp -Ldatum_amd/lib -ldatum_ocean_host -ldatum_ocean_hip -Wl,-rpath,'$$ORIGIN/../datum_amd/lib'

$(EXAMPLE): examples/ocean_headless.cpp $(HOSTLIB)
	$(CXX) -O2 -std=c++14 -Wall -o $@ examples/ocean_headless.cpp -Ldatum_amd/lib -ldatum_ocean_host -ldatum_ocean_hip -Wl,-rpath,'$$ORIGIN/../datum_amd/lib'

# CPU emulation of the thread-parallel line FFT, and the memory layouts walked point by point (tests only)
EMUL = tests/cpu/libfft_core_emul.so
emul: $(EMUL)

# (the layout walk is compiled in where the tests directory holds it: the library still builds for a tests directory without it)
EMULSRC = tests/cpu/fft_core_emul.cpp $(wildcard tests/cpu/layout_emul.cpp tests/cpu/writeback_emul.cpp tests/cpu/quadrant_emul.cpp) tests/cpu/phase_emul.cpp tests/cpu/body_emul.cpp tests/cpu/ray_emul.cpp tests/cpu/bounds_emul.cpp $(wildcard tests/cpu/velocity_emul.cpp) tests/cpu/drag_emul.cpp tests/cpu/step_emul.cpp tests/cpu/ripple_emul.cpp tests/cpu/couple_emul.cpp tests/cpu/rippled_emul.cpp tests/cpu/ripple_bounds_emul.cpp tests/cpu/ripple_foam_emul.cpp tests/cpu/ripple_deep_emul.cpp tests/cpu/ripple_wall_emul.cpp tests/cpu/ripple_bed_emul.cpp tests/cpu/ripple_swell_emul.cpp tests/cpu/contact_emul.cpp

# (-ffp-contract=off as the HIP module has it: the phase arithmetic is rounded as written)
$(EMUL): $(EMULSRC) datum_amd/csrc/ocean_fft_core.h datum_amd/csrc/ocean_layout.h datum_amd/csrc/ocean_writeback.h datum_amd/csrc/ocean_phase.h datum_amd/csrc/ocean_quadrant.h datum_amd/csrc/ocean_body.h datum_amd/csrc/ocean_ray.h datum_amd/csrc/ocean_bounds.h datum_amd/csrc/ocean_velocity.h datum_amd/csrc/ocean_drag.h datum_amd/csrc/ocean_step.h datum_amd/csrc/ocean_ripple.h datum_amd/csrc/ocean_couple.h datum_amd/csrc/ocean_rippled.h datum_amd/csrc/ocean_ripple_bounds.h datum_amd/csrc/ocean_ripple_foam.h datum_amd/csrc/ocean_ripple_deep.h datum_amd/csrc/ocean_ripple_wall.h datum_amd/csrc/ocean_ripple_bed.h datum_amd/csrc/ocean_ripple_swell.h datum_amd/csrc/ocean_contact.h include/datum_ocean_hip.h
	$(CXX) -O2 -std=c++17 -ffp-contract=off -fPIC -shared -o $@ $(EMULSRC)

# stand-in for the Vulkan side of the external-memory handshake (GPU tests only)
EXTMEM = tests/gpu/libextmem_helper.so
helpers: $(EXTMEM)

$(EXTMEM): tests/gpu/extmem_helper.hip
	$(HIPCC) -O2 -std=c++17 --offload-arch=$(ARCH) -fPIC -shared -o $@ tests/gpu/extmem_helper.hip

resource-usage: $(SRC) $(DEPS)
	$(HIPCC) $(HIPFLAGS) -Rpass-analysis=kernel-resource-usage -c -o /dev/null $(SRC) 2>&1 | grep -E "Function Name|VGPRs:|SGPRs:|Occupancy|LDS Size|ScratchSize" 

clean:
	rm -f $(LIB) $(HOSTLIB) $(STANDIN) $(EMUL) $(EXAMPLE) $(FARMEXAMPLE) $(EXTMEM)
	$(MAKE) -C oracle clean

.PHONY: all oracle emul helpers examples clean resource-usage
