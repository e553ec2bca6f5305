// SPV.cpp -- the sliding-DFT vocoder over the C ABI: Audio::convert_to_SPV / convert_to_ms_SPV (Conversions/AudioSPV.cpp:27-108),
// SPV::convert_to_audio / convert_to_lr_audio (:110-150), SPV::modify_frequency / repitch (SPV/SPV.cpp:21-44).
#include "flan/SPV.h"

#include <algorithm>
#include <iostream>
#include <utility>

#include "device_call.h"
#include "flan/Audio.h"

namespace flan {

using detail::DeviceCall;

SPV::SPV() : SPVBuffer() {}
SPV::SPV( SPVBuffer && other ) : SPVBuffer( std::move( other ) ) {}
SPV::SPV( const Format & f ) : SPVBuffer( f ) {}
SPV SPV::copy() const { return SPVBuffer::copy(); }

SPV Audio::convert_to_SPV( Bin dft_size, flan_CANCEL_ARG_CPP ) const
	{
	if( is_null() || dft_size < 2 ) return SPV();
	if( canceller ) return SPV();
	SPVBuffer::Format f;                                       // AudioSPV.cpp:30-35
	f.num_channels = get_num_channels();
	f.num_frames = get_num_frames();
	f.num_bins = dft_size;
	f.sample_rate = get_sample_rate();
	const float * d_audio = device_data();
	if( !d_audio ) return SPV();
	DeviceCall call( "convert_to_SPV" );
	flanhip_MF * d_spv = call.output<flanhip_MF>( size_t( f.num_channels ) * size_t( f.num_frames ) * size_t( f.num_bins ) );
	if( !d_spv ) return SPV();
	if( !call.launch( flanhip_spv_analyze_dev( d_audio, f.num_channels, f.num_frames, f.sample_rate, f.num_bins, d_spv, nullptr ) ) ) return SPV();
	if( call.wait( canceller ) == FLANHIP_ERR_CANCELLED || canceller ) return SPV();
	return call.finish<SPVBuffer>( f );
	}

SPV Audio::convert_to_ms_SPV( Bin dft_size, flan_CANCEL_ARG_CPP ) const
	{
	return convert_to_mid_side().convert_to_SPV( dft_size, canceller );
	}

Audio SPV::convert_to_audio( flan_CANCEL_ARG_CPP ) const
	{
	if( is_null() || get_num_bins() < 2 ) return Audio::create_null();
	if( canceller ) return Audio::create_null();
	AudioBuffer::Format af;                                    // AudioSPV.cpp:114-117
	af.num_channels = get_num_channels();
	af.num_frames = get_num_frames();
	af.sample_rate = get_sample_rate();
	const MF * d_spv = device_data();
	if( !d_spv ) return Audio::create_null();
	DeviceCall call( "SPV::convert_to_audio" );
	float * out = call.output<float>( size_t( af.num_channels ) * size_t( af.num_frames ) );
	// (a shape the device does not take is the launch's to refuse and report: no 0 bytes reach the skeleton)
	void * ws = call.workspace( std::max<size_t>( flanhip_spv_synthesize_workspace_bytes( get_num_channels(), get_num_frames(), get_num_bins(), get_sample_rate() ), 1 ) );
	if( !call.ok() ) return Audio::create_null();
	if( !call.launch( flanhip_spv_synthesize_dev( reinterpret_cast<const flanhip_MF*>( d_spv ), get_num_channels(), get_num_frames(),
			get_num_bins(), get_sample_rate(), out, ws, nullptr ) ) ) return Audio::create_null();
	if( call.wait( canceller ) == FLANHIP_ERR_CANCELLED || canceller ) return Audio::create_null();
	AudioBuffer audio = call.finish<AudioBuffer>( af );
	if( !call.ok() ) return Audio::create_null();
	return Audio( std::move( audio ) );
	}

Audio SPV::convert_to_lr_audio( flan_CANCEL_ARG_CPP ) const
	{
	return convert_to_audio( canceller ).convert_to_left_right();
	}

namespace {
// f = c (multiply 0) or f * c (multiply 1) on the device, m unchanged
SPV modify_frequency_const( const SPV & in, float c, int multiply )
	{
	const MF * d_in = in.device_data();
	const size_t count = size_t( in.get_num_channels() ) * size_t( in.get_num_frames() ) * size_t( in.get_num_bins() );
	return detail::device_call<SPVBuffer, flanhip_MF>( "SPV::modify_frequency", in.get_format(), count, d_in != nullptr, detail::kNoWorkspace, [&]( flanhip_MF * out, void * )
		{
		return flanhip_spv_modify_frequency_const_dev( reinterpret_cast<const flanhip_MF*>( d_in ), in.get_num_channels(), in.get_num_frames(), in.get_num_bins(), c, multiply, out, nullptr );
		} );
	}
}

SPV SPV::modify_frequency( const Function<TF, Frequency> & mod ) const
	{
	if( is_null() ) return SPV();                              // SPV.cpp:23
	if( mod.is_constant() ) return modify_frequency_const( *this, mod.get_constant(), 0 );
	SPV out = copy();                                          // :25
	std::vector<MF> & data = out.get_buffer();
	for( Channel channel = 0; channel < get_num_channels(); ++channel )                 // :27-36, the callable at each MF's own (time, f)
		for( Frame frame = 0; frame < get_num_frames(); ++frame )
			{
			const Second time = frame_to_time( fFrame( frame ) );
			MF * row = data.data() + get_buffer_pos( channel, frame, 0 );
			for( Bin bin = 0; bin < get_num_bins(); ++bin ) row[bin].f = mod( TF{ time, row[bin].f } );
			}
	return out;
	}

SPV SPV::repitch( const Function<TF, Frequency> & mod ) const
	{
	if( is_null() ) return SPV();
	if( mod.is_constant() ) return modify_frequency_const( *this, mod.get_constant(), 1 );
	return modify_frequency( [&]( TF tf ){ return tf.f * mod( tf ); } );                // SPV.cpp:42-43
	}

} // namespace flan
