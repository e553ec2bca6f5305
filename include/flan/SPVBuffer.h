// flan/SPVBuffer.h -- sliding-DFT phase-vocoder container (mirrors the reference's src/flan/SPV/SPVBuffer.h and SPVBuffer.cpp).
//
// Layout: MF[channel][frame][bin], one frame per input sample: analysis rate = sample rate, bin b at b sr / num_bins.  Move-only, explicit
// copy().  Like PVBuffer, the data may live in HBM only (convert_to_SPV -> convert_to_audio never leaves it); the host copy is brought
// over on first use.  A buffer made from a Format is all zeros and takes no memory until it is touched.
#pragma once
#include <memory>
#include <vector>

#include "flan/defines.h"
#include "flan/mirror.h"

namespace flan {

class SPVBuffer
	{
public:
	struct Format
		{
		Channel num_channels = 0;
		Frame num_frames = 0;
		Bin num_bins = 0;
		FrameRate sample_rate = 48000;
		};

	SPVBuffer( const SPVBuffer & ) = delete;
	SPVBuffer( SPVBuffer && ) = default;
	SPVBuffer & operator=( const SPVBuffer & ) = delete;
	SPVBuffer & operator=( SPVBuffer && ) = default;
	~SPVBuffer() = default;

	SPVBuffer();
	explicit SPVBuffer( const Format & );

	SPVBuffer copy() const;
	bool is_null() const;                                                        // SPVBuffer.cpp: sample_rate <= 0 or no data
	void clear_buffer();

	const Format & get_format() const { return format; }
	Channel get_num_channels() const { return format.num_channels; }
	Frame get_num_frames() const { return format.num_frames; }
	Bin get_num_bins() const { return format.num_bins; }
	FrameRate get_sample_rate() const { return format.sample_rate; }
	FrameRate get_analysis_rate() const { return format.sample_rate; }         // one spectrum per sample
	fFrame time_to_frame( Second t ) const { return t * get_sample_rate(); }
	Second frame_to_time( fFrame f ) const { return f / get_sample_rate(); }
	fBin frequency_to_bin( Frequency f ) const { return f * float( get_num_bins() ) / get_sample_rate(); }
	Frequency bin_to_frequency( fBin b ) const { return b * get_sample_rate() / float( get_num_bins() ); }
	size_t get_buffer_pos( Channel c, Frame f, Bin b ) const                    // 64-bit here (the reference's int product overflows)
		{ return ( size_t( c ) * size_t( format.num_frames ) + size_t( f ) ) * size_t( format.num_bins ) + size_t( b ); }

	MF get_MF( Channel c, Frame f, Bin b ) const;
	MF & get_MF( Channel c, Frame f, Bin b );
	const std::vector<MF> & get_buffer() const { return mirror.host( count() ); }   // downloads from HBM on first use
	std::vector<MF> & get_buffer() { return mirror.host( count() ); }               // ... and drops the device copy (the host owns the truth)

	// ---- device residency (MI355X) ----
	bool is_device_resident() const { return mirror.is_device_resident(); }
	bool host_copy_is_current() const { return mirror.host_copy_is_current(); }
	const MF * device_data() const { return mirror.device_data( count() ); }     // uploads on first use; nullptr on failure
	std::shared_ptr<detail::DeviceBlock> device_block() const { return mirror.device_block( count() ); }
	static SPVBuffer adopt_device( const Format &, std::shared_ptr<detail::DeviceBlock> );

protected:
	size_t count() const { return size_t( format.num_channels ) * size_t( format.num_frames ) * size_t( format.num_bins ); }
	Format format;
	detail::Mirror<MF> mirror{ "SPV", true };      // the data: host vector + HBM copy (mirror.h); zeros are not allocated until touched
	};

} // namespace flan
