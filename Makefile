# Builds libacdsp.so (HIP engine, gfx950 only) in-tree and the CPU oracle.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
CSRC = ac_dsp_amd/csrc
OUT = ac_dsp_amd/lib/libacdsp.so
SRCS = $(CSRC)/engine.hip $(CSRC)/engine_fir.hip $(CSRC)/engine_cic.hip $(CSRC)/engine_ddc.hip $(CSRC)/engine_poly.hip $(CSRC)/engine_misc.hip $(CSRC)/fir_generic.hip $(CSRC)/fir_mfma.hip $(CSRC)/fir_mfma_mid.hip $(CSRC)/fir_mfma_mid2.hip $(CSRC)/fir_mfma_mid3.hip $(CSRC)/fir_mfma_alt.hip $(CSRC)/fir_mfma_alt2.hip $(CSRC)/fir_long.hip $(CSRC)/fir_s8.hip $(CSRC)/fir_gen.hip $(CSRC)/fir_gen_ring.hip $(CSRC)/fir_gen_ring_s8.hip $(CSRC)/fir_gen_cascade.hip $(CSRC)/fir_gen_cascade_s8.hip $(CSRC)/fir_gen_cascade_dec.hip $(CSRC)/fir_up.hip $(CSRC)/fir_up_b.hip $(CSRC)/fir_up_c.hip $(CSRC)/fir_up_s8.hip $(CSRC)/fir_up_s8_b.hip $(CSRC)/polydec.hip $(CSRC)/polydec_long.hip $(CSRC)/polydec_s8.hip $(CSRC)/polyintr.hip $(CSRC)/polyintr_long.hip $(CSRC)/intg_dump.hip $(CSRC)/mv_avg.hip $(CSRC)/mv_avg_s8.hip $(CSRC)/mv_avg_plan.hip $(CSRC)/cic.hip $(CSRC)/cic2.hip $(CSRC)/cic2_b.hip $(CSRC)/cic2_c.hip $(CSRC)/cic2_d.hip $(CSRC)/cic2_e.hip $(CSRC)/cic2_f.hip $(CSRC)/cic2_s8.hip $(CSRC)/cic2_s8_b.hip $(CSRC)/cic2_s8_c.hip $(CSRC)/wide.hip $(CSRC)/diag.hip $(CSRC)/node.hip
OBJS = $(SRCS:.hip=.o)
DEPS = $(OBJS:.o=.d)
HIPFLAGS = --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wall -Wno-unused-function

all: $(OUT) oracle

# header dependencies come from the compiler (-MMD writes a .d file beside every object)
%.o: %.hip
	$(HIPCC) $(HIPFLAGS) -MMD -MP -c $< -o $@

-include $(DEPS)

$(OUT): $(OBJS)
	@mkdir -p ac_dsp_amd/lib
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $(OBJS) -o $@

oracle:
	$(MAKE) -C oracle

clean:
	rm -f $(OBJS) $(DEPS) $(OUT)
	$(MAKE) -C oracle clean

.PHONY: all oracle clean
