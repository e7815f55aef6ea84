// TEST INFRASTRUCTURE.  A stand-in for libamdhip64 so that the HOST side of the product -- structure building, colouring, strip
// partition, incremental placement, the world chain's bookkeeping, the reference-side binding's pack / unpack -- can run under
// AddressSanitizer + UndefinedBehaviorSanitizer on a box without a GPU (tests/hostcheck/Makefile, tests/test_hostcheck.py).
// "Device" memory is heap memory (so an out-of-bounds hipMemcpy into a device table is an ASan report), copies are memcpy,
// graphs are inert handles, a stream or an event is a one-byte heap block that its destroy call frees (so one that is never destroyed
// is a leak and one destroyed twice an ASan report), and kernels are never run: hipLaunchKernel returns success and does nothing --
// with S2_HOSTCHECK_TRACE_LAUNCHES set it prints one line per launch first: "LAUNCH <kernel symbol> grid <x> block <x> lds <bytes>"
// (which kernel the host picked and the dynamic LDS it asked for are host decisions: tests/test_wide_island_kinds_host.py).
// While S2_HOSTCHECK_TRACE_CALLS is set (looked up at every call, so a program can switch it) the stub prints what a call sequence
// is made of, one line each and no pointers, so that two runs -- or two versions of the host code -- print the same text
// (tests/test_query_host.py):
//   LAUNCH <kernel> grid <x> <y> block <x> lds <bytes>            hipLaunchKernel (the demangled name with its template arguments)
//   COPY <kind> <bytes>                                           hipMemcpyAsync
//   MEMSET <value> <bytes>                                        hipMemsetAsync
//   SYNC                                                          hipStreamSynchronize
// While S2_HOSTCHECK_FAIL_MALLOC is set (looked up at every call as well) hipMalloc answers hipErrorOutOfMemory: how a program walks the
// paths behind a device block that cannot grow (ray_report_main.cpp, grid_report_main.cpp, actuators_main.cpp).
// Results of a step are therefore meaningless; what is checked is that the host code touches only memory it owns.
// The product never links this file.
#include <hip/hip_runtime_api.h>

#include <cxxabi.h>
#include <dlfcn.h>
#include <elf.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int s_dummy[16];
// the configuration of the `kernel<<<...>>>` in flight (clang's host code pushes it, the kernel's stub pops it and calls hipLaunchKernel)
static thread_local dim3 s_grid(1), s_block(1);
static thread_local size_t s_shared = 0;

static bool traceCalls()
{
	return getenv("S2_HOSTCHECK_TRACE_CALLS") != nullptr;
}

// The handle of a kernel in an unnamed namespace is a local symbol, which dladdr does not know: its name from the .symtab of the file
// it was loaded from (under ASan the handle has a second, longer name: the shortest is the kernel's own).
static const char* localSymbol(const char* file, const void* base, const void* fn)
{
	static std::string loaded;
	static std::vector<char> image;
	if (loaded != file)
	{
		loaded = file;
		image.clear();
		if (FILE* f = fopen(file, "rb"))
		{
			fseek(f, 0, SEEK_END);
			const long size = ftell(f);
			fseek(f, 0, SEEK_SET);
			image.resize(size > 0 ? (size_t)size : 0);
			if (fread(image.data(), 1, image.size(), f) != image.size())
			{
				image.clear();
			}
			fclose(f);
		}
	}
	if (image.size() < sizeof(Elf64_Ehdr) || memcmp(image.data(), ELFMAG, SELFMAG) != 0)
	{
		return nullptr;
	}
	const Elf64_Ehdr* header = (const Elf64_Ehdr*)image.data();
	const Elf64_Shdr* sections = (const Elf64_Shdr*)(image.data() + header->e_shoff);
	const Elf64_Addr want = (Elf64_Addr)((const char*)fn - (const char*)base);
	const char* best = nullptr;
	for (int i = 0; i < header->e_shnum; ++i)
	{
		if (sections[i].sh_type != SHT_SYMTAB)
		{
			continue;
		}
		const Elf64_Sym* symbols = (const Elf64_Sym*)(image.data() + sections[i].sh_offset);
		const char* names = image.data() + sections[sections[i].sh_link].sh_offset;
		for (size_t k = 0; k < sections[i].sh_size / sizeof(Elf64_Sym); ++k)
		{
			const char* name = names + symbols[k].st_name;
			if (symbols[k].st_value == want && ELF64_ST_TYPE(symbols[k].st_info) == STT_OBJECT && (best == nullptr || strlen(name) < strlen(best)))
			{
				best = name;
			}
		}
	}
	return best;
}

// a kernel's symbol as the trace names it: demangled, without "void ", the unnamed namespace and the parameter list
static std::string kernelName(const char* symbol)
{
	if (symbol == nullptr)
	{
		return "?";
	}
	std::string name(symbol);
	const size_t alias = name.find("__sanitized_padded_global");
	if (alias != std::string::npos)
	{
		name.resize(alias);
	}
	int status = 0;
	if (char* plain = abi::__cxa_demangle(name.c_str(), nullptr, nullptr, &status))
	{
		name = plain;
		free(plain);
	}
	for (const char* drop : {"void ", "(anonymous namespace)::"})
	{
		for (size_t at = name.find(drop); at != std::string::npos; at = name.find(drop))
		{
			name.erase(at, strlen(drop));
		}
	}
	return name.substr(0, name.find('('));
}

static const char* copyKind(hipMemcpyKind kind)
{
	switch (kind)
	{
		case hipMemcpyHostToHost:
			return "HostToHost";
		case hipMemcpyHostToDevice:
			return "HostToDevice";
		case hipMemcpyDeviceToHost:
			return "DeviceToHost";
		case hipMemcpyDeviceToDevice:
			return "DeviceToDevice";
		default:
			return "Default";
	}
}

extern "C" {

hipError_t hipGetDeviceCount(int* count)
{
	*count = 1;
	return hipSuccess;
}
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetDevice(int* device)
{
	*device = 0;
	return hipSuccess;
}
hipError_t hipDeviceSynchronize(void) { return hipSuccess; }
int hipGetStreamDeviceId(hipStream_t) { return 0; }
hipError_t hipGetDevicePropertiesR0600(hipDeviceProp_tR0600* prop, int)
{
	memset(prop, 0, sizeof(*prop));
	prop->multiProcessorCount = 256, prop->warpSize = 64, prop->maxThreadsPerBlock = 1024;
	strcpy(prop->gcnArchName, "gfx950:sramecc+:xnack-");
	prop->sharedMemPerBlock = 160 * 1024, prop->regsPerBlock = 131072;
	return hipSuccess;
}
hipError_t hipDeviceGetAttribute(int* value, hipDeviceAttribute_t attr, int)
{
	*value = attr == hipDeviceAttributeMultiprocessorCount ? 256 : attr == hipDeviceAttributeWarpSize ? 64 : 1024;
	return hipSuccess;
}
hipError_t hipDeviceGetPCIBusId(char* pciBusId, int len, int)
{
	strncpy(pciBusId, "0000:00:00.0", (size_t)len);
	return hipSuccess;
}
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipPeekAtLastError(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "hip_stub"; }
const char* hipGetErrorName(hipError_t) { return "hip_stub"; }

hipError_t hipMalloc(void** ptr, size_t size)
{
	if (getenv("S2_HOSTCHECK_FAIL_MALLOC") != nullptr)
	{
		*ptr = nullptr;
		return hipErrorOutOfMemory;
	}
	*ptr = calloc(size ? size : 1, 1);
	return *ptr ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipFree(void* ptr)
{
	free(ptr);
	return hipSuccess;
}
hipError_t hipHostMalloc(void** ptr, size_t size, unsigned int)
{
	*ptr = calloc(size ? size : 1, 1);
	return *ptr ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipHostFree(void* ptr)
{
	free(ptr);
	return hipSuccess;
}
hipError_t hipHostGetDevicePointer(void** devPtr, void* hstPtr, unsigned int)
{
	*devPtr = hstPtr;
	return hipSuccess;
}
hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind)
{
	if (bytes)
	{
		memmove(dst, src, bytes);
	}
	return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t)
{
	if (traceCalls())
	{
		printf("COPY %s %zu\n", copyKind(kind), bytes);
		fflush(stdout);
	}
	if (bytes)
	{
		memmove(dst, src, bytes);
	}
	return hipSuccess;
}
hipError_t hipMemset(void* dst, int value, size_t bytes)
{
	if (bytes)
	{
		memset(dst, value, bytes);
	}
	return hipSuccess;
}
hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t)
{
	if (traceCalls())
	{
		printf("MEMSET %d %zu\n", value, bytes);
		fflush(stdout);
	}
	if (bytes)
	{
		memset(dst, value, bytes);
	}
	return hipSuccess;
}

hipError_t hipStreamCreateWithFlags(hipStream_t* stream, unsigned int)
{
	*stream = (hipStream_t)malloc(1);
	return hipSuccess;
}
hipError_t hipStreamCreate(hipStream_t* stream)
{
	*stream = (hipStream_t)malloc(1);
	return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t stream)
{
	free(stream);
	return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t)
{
	if (traceCalls())
	{
		printf("SYNC\n");
		fflush(stdout);
	}
	return hipSuccess;
}
hipError_t hipStreamQuery(hipStream_t) { return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned int) { return hipSuccess; }
hipError_t hipMemcpyPeerAsync(void* dst, int, const void* src, int, size_t bytes, hipStream_t)
{
	if (bytes)
	{
		memmove(dst, src, bytes);
	}
	return hipSuccess;
}
hipError_t hipDeviceCanAccessPeer(int* can, int, int)
{
	*can = 0;
	return hipSuccess;
}
hipError_t hipDeviceEnablePeerAccess(int, unsigned int) { return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t* event)
{
	*event = (hipEvent_t)malloc(1);
	return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* event, unsigned)
{
	*event = (hipEvent_t)malloc(1);
	return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t event)
{
	free(event);
	return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t)
{
	*ms = 0.0f;
	return hipSuccess;
}
hipError_t hipStreamBeginCapture(hipStream_t, hipStreamCaptureMode) { return hipSuccess; }
hipError_t hipStreamEndCapture(hipStream_t, hipGraph_t* graph)
{
	*graph = (hipGraph_t)s_dummy;
	return hipSuccess;
}
hipError_t hipGraphInstantiate(hipGraphExec_t* exec, hipGraph_t, hipGraphNode_t*, char*, size_t)
{
	*exec = (hipGraphExec_t)s_dummy;
	return hipSuccess;
}
hipError_t hipGraphLaunch(hipGraphExec_t, hipStream_t) { return hipSuccess; }
hipError_t hipGraphDestroy(hipGraph_t) { return hipSuccess; }
hipError_t hipGraphExecDestroy(hipGraphExec_t) { return hipSuccess; }
hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int) { return hipSuccess; }
hipError_t hipFuncGetAttributes(hipFuncAttributes* attr, const void*)
{
	memset(attr, 0, sizeof(*attr));
	attr->maxThreadsPerBlock = 1024;
	return hipSuccess;
}
hipError_t hipOccupancyMaxActiveBlocksPerMultiprocessor(int* numBlocks, const void*, int, size_t)
{
	*numBlocks = 1;
	return hipSuccess;
}

// what clang's host-side code for `kernel<<<...>>>(...)` and for a translation unit with kernels calls
hipError_t hipLaunchKernel(const void* fn, dim3 grid, dim3 block, void**, size_t shared, hipStream_t)
{
	static const bool trace = getenv("S2_HOSTCHECK_TRACE_LAUNCHES") != nullptr;
	if (trace)
	{
		Dl_info info;
		const bool named = dladdr(fn, &info) != 0 && info.dli_sname != nullptr && info.dli_saddr == fn;
		// (under ASan a kernel's handle has a second symbol, <name>__sanitized_padded_global: print the kernel's own)
		const char* alias = named ? strstr(info.dli_sname, "__sanitized_padded_global") : nullptr;
		printf("LAUNCH %.*s grid %u block %u lds %zu\n", alias != nullptr ? (int)(alias - info.dli_sname) : 1 << 20, named ? info.dli_sname : "?", grid.x, block.x, shared);
		fflush(stdout);
	}
	if (traceCalls())
	{
		Dl_info info;
		const char* name = nullptr;
		if (dladdr(fn, &info) != 0)
		{
			name = info.dli_sname != nullptr && info.dli_saddr == fn ? info.dli_sname : localSymbol(info.dli_fname, info.dli_fbase, fn);
		}
		printf("LAUNCH %s grid %u %u block %u lds %zu\n", kernelName(name).c_str(), grid.x, grid.y, block.x, shared);
		fflush(stdout);
	}
	return hipSuccess;
}
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t shared, hipStream_t)
{
	s_grid = grid, s_block = block, s_shared = shared;
	return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* shared, hipStream_t* stream)
{
	*grid = s_grid, *block = s_block, *shared = s_shared, *stream = nullptr;
	return hipSuccess;
}
void** __hipRegisterFatBinary(const void*) { return (void**)s_dummy; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void*, char*, const char*, unsigned int, void*, void*, void*, void*, int*) {}
void __hipRegisterVar(void**, void*, char*, const char*, int, size_t, int, int) {}
void __hipRegisterManagedVar(void*, void*, void*, const char*, size_t, unsigned) {}
}
